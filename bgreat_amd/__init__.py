"""bgreat_amd -- ctypes view of the C-ABI in include/bgreat_gpu.h (lib/libbgreat_gpu.so).

The product is the shared library + the `bgreat` CLI (C++/HIP).  This module only lets Python (tests,
bench.py, __graft_entry__) call the same entry points; it contains no algorithm and no CPU fallback: if
the library is missing it raises, and mapping calls fail when there is no HIP device.
"""
import ctypes as C
import importlib.util
import os
import subprocess
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BGR_LIB_PATH") or os.path.join(_HERE, "lib", "libbgreat_gpu.so")  # (the override: A/B builds of the kernels, tools only)
CLI_PATH = os.path.join(_HERE, "bin", "bgreat")

MODE_GREEDY, MODE_EXHAUSTIVE, MODE_ANCHORS = 0, 1, 2
ST_NOANCHOR, ST_FAILED, ST_ALIGNED, ST_MASK, ST_RC = 0, 1, 2, 3, 4
BUILD_ANCHORS = 1
BUILD_NO_EVICTIONS = 2  # test hook: keys whose two buckets are full go to the fallback list

# every symbol include/bgreat_gpu.h declares (checked by tests/test_cabi.py)
SYMBOLS = [
    "bgr_last_error", "bgr_device_count", "bgr_graph_build", "bgr_graph_build_from_fasta", "bgr_graph_blob",
    "bgr_graph_from_blob", "bgr_graph_info", "bgr_graph_jump_index", "bgr_graph_destroy", "bgr_graph_upload", "bgr_graph_device_blob",
    "bgr_graph_adopt_device_blob", "bgr_aligner_create", "bgr_aligner_destroy", "bgr_align_batch", "bgr_align_device", "bgr_aligner_path_stats",
    "bgr_aligner_sync", "bgr_aligner_device_results", "bgr_aligner_arena_ints", "bgr_aligner_fetch", "bgr_aligner_counters",
    "bgr_aligner_reset_counters", "bgr_aligner_kernel_time", "bgr_aligner_reset_kernel_time", "bgr_aligner_launch_info",
    "bgr_aligner_configure", "bgr_readset_load", "bgr_readset_count", "bgr_readset_view", "bgr_readset_destroy",
    "bgr_write_records", "bgr_graph_unitigs", "bgr_readset_load_parallel", "bgr_align_all", "bgr_host_alloc", "bgr_host_free",
    "bgr_set_build_threads", "bgr_graph_build_ex", "bgr_graph_build_from_fasta_ex", "bgr_graph_anchor_lookup", "bgr_graph_key_lookup", "bgr_graph_key_lookup_wide",
    "bgr_aligner_set_knob", "bgr_aligner_pass_counts", "bgr_aligner_last_pass_runs", "bgr_set_option", "bgr_get_option", "bgr_option_name", "bgr_plan_launch", "bgr_aligner_kernel_times", "bgr_devices_init", "bgr_devices_method", "bgr_packed_plane_words", "bgr_pack_reads", "bgr_align_batch_packed",
    "bgr_align_fasta_text", "bgr_aligner_fetch_text", "bgr_host_cache_release", "bgr_device_local_cpus", "bgr_text_stage_create", "bgr_text_stage_destroy", "bgr_text_stage_upload",
    "bgr_align_batch_begin", "bgr_align_batch_test", "bgr_align_batch_wait", "bgr_text_stage_device", "bgr_text_stage_upload_parts",
    "bgr_device_alloc", "bgr_device_free", "bgr_device_upload", "bgr_device_download",
    "bgr_aligner_abundance_enable", "bgr_aligner_abundance", "bgr_aligner_reset_abundance", "bgr_aligner_abundance_plan", "bgr_plan_abundance", "bgr_graph_abundance", "bgr_write_abundance",
    "bgr_aligner_links_enable", "bgr_aligner_links", "bgr_aligner_reset_links", "bgr_aligner_links_info", "bgr_aligner_links_plan", "bgr_plan_links", "bgr_graph_links_bound",
    "bgr_graph_links_enable", "bgr_graph_links", "bgr_write_gfa", "bgr_link_canonical", "bgr_graph_links_enabled",
    "bgr_links_bubbles", "bgr_aligner_bubbles", "bgr_aligner_bubbles_times", "bgr_graph_bubbles_enable", "bgr_graph_bubbles_enabled", "bgr_graph_bubbles", "bgr_write_bubbles",
    "bgr_aligner_triples_enable", "bgr_aligner_triples", "bgr_aligner_reset_triples", "bgr_aligner_triples_info", "bgr_triple_canonical", "bgr_graph_triples_bound",
    "bgr_graph_triples_enable", "bgr_graph_triples_enabled", "bgr_graph_triples", "bgr_write_triples",
    "bgr_bubbles_phase", "bgr_graph_phase_enable", "bgr_graph_phase_enabled", "bgr_graph_phase", "bgr_write_phase",
    "bgr_phase_blocks", "bgr_phase_blocks_times", "bgr_graph_blocks_enable", "bgr_graph_blocks_enabled", "bgr_graph_blocks", "bgr_write_blocks",
    "bgr_blocks_haplotypes", "bgr_blocks_haplotypes_times", "bgr_graph_haplotypes_enable", "bgr_graph_haplotypes_enabled", "bgr_graph_haplotypes", "bgr_write_haplotypes",
    "bgr_graph_recompact", "bgr_graph_recompact_times", "bgr_graph_recompact_enable", "bgr_graph_recompact_enabled", "bgr_graph_recompact_result", "bgr_write_recompact",
    "bgr_blocks_tag_table", "bgr_read_blocks_tags", "bgr_aligner_haplotag_enable", "bgr_aligner_haplotags", "bgr_graph_haplotag_enable", "bgr_graph_haplotag_enabled",
    "bgr_aligner_path_diffs", "bgr_aligner_gaf_cs_enable", "bgr_graph_gaf_cs_enable", "bgr_graph_gaf_cs_enabled",
    "bgr_aligner_pileup_enable", "bgr_aligner_pileup", "bgr_aligner_reset_pileup", "bgr_graph_pileup_enable", "bgr_graph_pileup_enabled", "bgr_graph_pileup",
    "bgr_write_pileup", "bgr_write_depth",
    "bgr_aligner_pileup_sites", "bgr_aligner_pileup_sites_times", "bgr_aligner_pileup_add", "bgr_graph_variants_enable", "bgr_graph_variants_enabled", "bgr_graph_variants",
    "bgr_graph_variants_params", "bgr_write_vcf", "bgr_parse_af_ppm",
    "bgr_aligner_pileup_strands_enable", "bgr_aligner_pileup_forward", "bgr_aligner_pileup_strand_sites", "bgr_graph_pileup_strands_enable", "bgr_graph_pileup_strands_enabled",
    "bgr_graph_pileup_forward", "bgr_graph_variants_strands_enable", "bgr_graph_variant_strand_sites", "bgr_write_pileup_strands", "bgr_write_vcf_strands", "bgr_parse_min_alt_strand",
    "bgr_graph_inside_build", "bgr_graph_inside_info", "bgr_graph_inside_lookup", "bgr_aligner_inside_enable", "bgr_aligner_inside_count",
    "bgr_graph_inside_enable", "bgr_graph_inside_enabled", "bgr_graph_inside_count",
    "bgr_aligner_exhaustive_paths_enable", "bgr_aligner_device_rows_view", "bgr_graph_exhaustive_paths_enable", "bgr_graph_exhaustive_paths_enabled",
]
KNOB_EXH_FRAME_CAP, KNOB_EXH_SEARCH, KNOB_BATCH_SPLIT_LIMIT, KNOB_DEBUG_STOP, KNOB_GREEDY_FAST, KNOB_EXH_FAST, KNOB_ANCHORS_FAST, KNOB_BATCH_OVERLAP, KNOB_EXH_MEMO_CAP, KNOB_GREEDY_PREPASS, KNOB_KERNEL_EVENTS = 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11
KNOB_ABUNDANCE_FORM = 12
ABUNDANCE_AUTO, ABUNDANCE_GLOBAL, ABUNDANCE_LDS = 0, 1, 2
KNOB_LINKS_FORM = 13
LINKS_AUTO, LINKS_GLOBAL, LINKS_LDS = 0, 1, 2
KNOB_DEVICE_OVERLAP = 14
KNOB_GREEDY_JUMP = 15
JUMP_ABSENT = ("", "two-word overlap keys", "unitig bases outside ACGT", "key table not staged in LDS", "index beyond the cache cap",
               "an interior (k-1)-mer of a unitig is an overlap key, or built with build_jump = 0")
SEARCH_AUTO, SEARCH_DEPTH_FIRST, SEARCH_BY_LEVEL = 0, 1, 2


class _Borrowed(np.ndarray):
    """ndarray view of library-owned memory; `_owner` pins the handle that owns it."""
    _owner = None


class PlanInput(C.Structure):  # bgr_plan_input
    _fields_ = [("k", C.c_uint32), ("slot_fill_x100", C.c_uint32), ("table_bytes", C.c_uint32), ("has_exceptions", C.c_uint32), ("anchors", C.c_uint32), ("anchor_levels", C.c_uint32),
                ("graph_bases", C.c_uint64), ("n_unitigs", C.c_uint64), ("max_unitig_len", C.c_uint64),
                ("num_cus", C.c_uint32), ("resident_waves", C.c_uint32 * 7), ("lds_per_cu", C.c_uint64),
                ("cfg_waves", C.c_uint32), ("cfg_blocks_per_cu", C.c_uint32), ("cfg_lds_mphf", C.c_uint32),
                ("mode", C.c_uint32), ("max_mismatch", C.c_uint32), ("partial", C.c_uint32), ("max_read_len", C.c_uint32),
                ("n_reads", C.c_uint64), ("total_bases", C.c_uint64), ("wide_keys", C.c_uint32), ("reserved0", C.c_uint32)]


class PlanPass(C.Structure):
    _fields_ = [("used", C.c_uint32), ("blocks", C.c_uint32), ("waves_per_block", C.c_uint32), ("lds_bytes", C.c_uint32), ("table_staged", C.c_uint32)]


class PlanOutput(C.Structure):  # bgr_plan_output
    _fields_ = [("pass_", PlanPass * 6), ("level_search", C.c_uint32), ("deep_only", C.c_uint32), ("x4_levels", C.c_uint32), ("memo_cap", C.c_uint32),
                ("deep_scratch_bytes", C.c_uint64), ("arena_ints", C.c_uint64)]


class BgrError(RuntimeError):
    pass


class Params(C.Structure):
    _fields_ = [("mode", C.c_uint32), ("max_mismatch", C.c_uint32), ("effort", C.c_uint32), ("partial", C.c_uint32)]


class RunOptions(C.Structure):
    _fields_ = [("struct_size", C.c_uint64), ("n_gpus", C.c_uint32), ("threads", C.c_uint32), ("batch_reads", C.c_uint64), ("chunk_bytes", C.c_uint64),
                ("fastq", C.c_uint32), ("write_exhaustive", C.c_uint32), ("echo_files", C.c_uint32), ("correction", C.c_uint32),
                ("no_overlap_file", C.c_char_p), ("first_device", C.c_uint32), ("route", C.c_uint32), ("numa", C.c_uint32), ("split_output", C.c_uint32), ("gaf", C.c_uint32),
                ("abundance", C.c_uint32)]


class UnitigAbundance(C.Structure):  # bgr_unitig_abundance
    _fields_ = [("reads", C.c_uint64), ("bases", C.c_uint64), ("kmers", C.c_uint64)]


class Link(C.Structure):  # bgr_link
    _fields_ = [("from_", C.c_int32), ("to", C.c_int32), ("count", C.c_uint64)]


LINK_DTYPE = np.dtype([("from", np.int32), ("to", np.int32), ("count", np.uint64)])   # an array of bgr_link


class Bubble(C.Structure):  # bgr_bubble
    _fields_ = [("source", C.c_int32), ("sink", C.c_int32), ("branch", C.c_int32 * 2), ("count", C.c_uint64 * 4)]


BUBBLE_DTYPE = np.dtype([("source", np.int32), ("sink", np.int32), ("branch", np.int32, (2,)), ("count", np.uint64, (4,))])   # an array of bgr_bubble
BUBBLES_TILE = 1024   # BGR_BUBBLES_TILE: oriented ids per tile of the count and emit passes


class Triple(C.Structure):  # bgr_triple
    _fields_ = [("from_", C.c_int32), ("via", C.c_int32), ("to", C.c_int32), ("reserved", C.c_int32), ("count", C.c_uint64)]


TRIPLE_DTYPE = np.dtype([("from", np.int32), ("via", np.int32), ("to", np.int32), ("reserved", np.int32), ("count", np.uint64)])   # an array of bgr_triple


class Phase(C.Structure):  # bgr_phase
    _fields_ = [("via", C.c_int32), ("source", C.c_int32), ("in_", C.c_int32 * 2), ("out", C.c_int32 * 2), ("sink", C.c_int32), ("reserved", C.c_int32), ("count", C.c_uint64 * 4)]


PHASE_DTYPE = np.dtype([("via", np.int32), ("source", np.int32), ("in", np.int32, (2,)), ("out", np.int32, (2,)), ("sink", np.int32), ("reserved", np.int32),
                        ("count", np.uint64, (4,))])   # an array of bgr_phase


class BlockEntry(C.Structure):  # bgr_block_entry
    _fields_ = [("block", C.c_uint32), ("index", C.c_uint32), ("size", C.c_uint32), ("bubble", C.c_uint32), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


BLOCK_DTYPE = np.dtype([("block", np.uint32), ("index", np.uint32), ("size", np.uint32), ("bubble", np.uint32), ("flags", np.uint32), ("reserved", np.uint32)])   # an array of bgr_block_entry
BLOCK_REVERSED, BLOCK_HAP, BLOCK_CIRCULAR, BLOCK_CONFLICT = 1, 2, 4, 8
BLOCKS_TILE = 1024   # BGR_BLOCKS_TILE: nodes per tile of the count and place passes


class Haplotype(C.Structure):  # bgr_haplotype
    _fields_ = [("block", C.c_uint32), ("hap", C.c_uint32), ("size", C.c_uint32), ("flags", C.c_uint32), ("offset", C.c_uint64), ("length", C.c_uint64)]


CHAIN_DTYPE = np.dtype([("seq_off", np.uint64), ("seq_len", np.uint64), ("walk_off", np.uint64), ("n_unitigs", np.uint32), ("flags", np.uint32)])   # an array of bgr_chain
CHAIN_CIRCULAR = 1
HAPLOTYPE_DTYPE = np.dtype([("block", np.uint32), ("hap", np.uint32), ("size", np.uint32), ("flags", np.uint32), ("offset", np.uint64), ("length", np.uint64)])   # an array of bgr_haplotype


class PathStat(C.Structure):  # bgr_path_stat
    _fields_ = [("path_len", C.c_uint64), ("path_start", C.c_uint64), ("aligned", C.c_uint32), ("mismatches", C.c_uint32)]


PATH_STAT_NO_WALK = 0x80000000
PATH_DIFF_DTYPE = np.dtype([("read_pos", np.uint32), ("path_base", np.uint8), ("read_base", np.uint8), ("reserved", np.uint16)])   # an array of bgr_path_diff


class InsideInfo(C.Structure):  # bgr_inside_info
    _fields_ = [("entries", C.c_uint64), ("slots", C.c_uint64), ("bytes", C.c_uint64), ("build_seconds", C.c_double)]


class Ticket(C.Structure):
    _fields_ = [("aligner", C.c_void_p), ("n_reads", C.c_uint64), ("serial", C.c_uint64)]


class TextBatch(C.Structure):
    _fields_ = [("struct_size", C.c_uint64), ("text", C.c_void_p), ("text_bytes", C.c_uint64), ("want_output", C.c_uint32), ("irregular", C.c_uint32), ("paths_out", C.c_void_p),
                ("paths_cap", C.c_uint64), ("notaligned_out", C.c_void_p), ("notaligned_cap", C.c_uint64), ("n_records", C.c_uint64),
                ("n_accepted", C.c_uint64), ("paths_bytes", C.c_uint64), ("notaligned_bytes", C.c_uint64), ("stage", C.c_void_p),
                ("fastq", C.c_uint32), ("reserved", C.c_uint32), ("record_info_out", C.c_void_p), ("record_info_cap", C.c_uint64)]


class PackedReads(C.Structure):
    _fields_ = [("read_offsets", C.c_void_p), ("fw3", C.c_void_p), ("hasn", C.c_void_p), ("nm_index", C.c_void_p), ("nm_value", C.c_void_p),
                ("nm_count", C.c_uint64), ("max_read_len", C.c_uint32)]


class GraphInfo(C.Structure):
    _fields_ = [("k", C.c_uint32), ("n_levels", C.c_uint32), ("n_unitigs", C.c_uint64), ("n_keys", C.c_uint64),
                ("n_left_keys", C.c_uint64), ("n_right_keys", C.c_uint64), ("n_fallback", C.c_uint64),
                ("total_bases", C.c_uint64), ("blob_bytes", C.c_uint64), ("mphf_bytes", C.c_uint64),
                ("max_unitig_len", C.c_uint64), ("has_exceptions", C.c_uint32), ("has_anchors", C.c_uint32),
                ("gamma", C.c_double), ("jump_entries", C.c_uint64), ("jump_bytes", C.c_uint64), ("jump_stride", C.c_uint32), ("jump_absent", C.c_uint32),
                ("jump_dropped_x1000", C.c_uint32), ("reserved", C.c_uint32)]


_lib = None


def build(force=False):
    """Compile lib/libbgreat_gpu.so and bin/bgreat for gfx950 (hipcc cross-compiles without a GPU)."""
    if force:
        subprocess.check_call(["make", "-C", _HERE, "clean"])
    subprocess.check_call(["make", "-s", "-C", _HERE, "all"])


def _pin_hip_runtime():
    """PyTorch-ROCm wheels bundle their own libamdhip64.so.7 (same SONAME as /opt/rocm's): whichever is loaded
    first serves the whole process.  Device pointers only make sense inside ONE runtime, so when torch is
    installed its copy is loaded first (without importing torch); a later `import torch` then shares it."""
    if "torch" in sys.modules or os.environ.get("BGREAT_SYSTEM_HIP"):
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec and spec.submodule_search_locations:
        p = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
        if os.path.exists(p):
            C.CDLL(p, mode=C.RTLD_GLOBAL)


def lib():
    global _lib
    if _lib is not None:
        return _lib
    _pin_hip_runtime()
    if not os.path.exists(LIB_PATH):
        raise BgrError("libbgreat_gpu.so is not built (%s); run `make -C bgreat_amd` -- there is no fallback path" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp, u64, u32, i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
    L.bgr_last_error.restype = C.c_char_p
    L.bgr_set_build_threads.restype = None
    L.bgr_set_build_threads.argtypes = [C.c_uint32]
    L.bgr_device_count.restype = i32
    L.bgr_graph_build.argtypes = [u32, u64, vp, vp, C.c_double, C.POINTER(vp)]
    L.bgr_graph_build_from_fasta.argtypes = [C.c_char_p, u32, C.c_double, C.POINTER(vp)]
    L.bgr_graph_build_ex.argtypes = [u32, u64, vp, vp, C.c_double, u32, C.POINTER(vp)]
    L.bgr_graph_build_from_fasta_ex.argtypes = [C.c_char_p, u32, C.c_double, u32, C.POINTER(vp)]
    L.bgr_graph_anchor_lookup.argtypes = [vp, u64, C.POINTER(u64), C.POINTER(u64)]
    L.bgr_graph_key_lookup.argtypes = [vp, u64, C.POINTER(C.c_uint32)]
    L.bgr_graph_key_lookup_wide.argtypes = [vp, u64, u64, C.POINTER(C.c_uint32)]
    L.bgr_graph_blob.restype = vp
    L.bgr_graph_blob.argtypes = [vp, C.POINTER(u64)]
    L.bgr_graph_from_blob.argtypes = [vp, u64, C.POINTER(vp)]
    L.bgr_graph_info.argtypes = [vp, C.POINTER(GraphInfo)]
    L.bgr_graph_unitigs.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(u64)]
    L.bgr_graph_destroy.argtypes = [vp]
    L.bgr_graph_destroy.restype = None
    L.bgr_graph_upload.argtypes = [vp, i32]
    L.bgr_graph_device_blob.restype = vp
    L.bgr_graph_device_blob.argtypes = [vp, i32]
    L.bgr_graph_adopt_device_blob.argtypes = [i32, vp, u64, C.POINTER(vp)]
    L.bgr_devices_init.argtypes = [vp, i32, u32, u32]
    L.bgr_devices_method.argtypes = [vp]
    L.bgr_devices_method.restype = u32
    L.bgr_aligner_create.argtypes = [vp, i32, C.POINTER(vp)]
    L.bgr_aligner_destroy.argtypes = [vp]
    L.bgr_aligner_destroy.restype = None
    L.bgr_align_batch.argtypes = [vp, C.POINTER(Params), vp, vp, u64, vp, u64, vp, vp]
    L.bgr_align_device.argtypes = [vp, C.POINTER(Params), vp, vp, u64, u64, u32]
    L.bgr_packed_plane_words.argtypes = [u64, u64]
    L.bgr_packed_plane_words.restype = u64
    L.bgr_pack_reads.argtypes = [vp, vp, u64, vp, vp, vp, vp, u64, C.POINTER(u64), C.POINTER(u32)]
    L.bgr_align_batch_packed.argtypes = [vp, C.POINTER(Params), C.POINTER(PackedReads), u64, vp, u64, vp, vp]
    L.bgr_align_fasta_text.argtypes = [vp, C.POINTER(Params), C.POINTER(TextBatch)]
    L.bgr_align_batch_begin.argtypes = [vp, C.POINTER(Params), vp, vp, u64, C.POINTER(Ticket)]
    L.bgr_align_batch_test.argtypes = [C.POINTER(Ticket)]
    L.bgr_align_batch_wait.argtypes = [C.POINTER(Ticket), vp, u64, vp, vp]
    L.bgr_aligner_fetch_text.argtypes = [vp, C.POINTER(TextBatch)]
    L.bgr_text_stage_create.argtypes = [C.c_int, C.POINTER(vp)]
    L.bgr_text_stage_destroy.argtypes = [vp]
    L.bgr_text_stage_destroy.restype = None
    L.bgr_text_stage_upload.argtypes = [vp, vp, u64]
    L.bgr_aligner_sync.argtypes = [vp]
    L.bgr_aligner_device_results.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    L.bgr_aligner_arena_ints.argtypes = [vp, vp]
    L.bgr_aligner_fetch.argtypes = [vp, u64, vp, u64, vp, vp]
    L.bgr_aligner_path_stats.argtypes = [vp, vp, vp, u64, vp]
    L.bgr_aligner_counters.argtypes = [vp, vp]
    L.bgr_aligner_reset_counters.argtypes = [vp]
    L.bgr_aligner_kernel_time.argtypes = [vp, C.POINTER(u64), C.POINTER(C.c_double)]
    L.bgr_aligner_reset_kernel_time.argtypes = [vp]
    L.bgr_aligner_kernel_times.argtypes = [vp, C.POINTER(u64), vp, vp]
    L.bgr_aligner_launch_info.argtypes = [vp, vp]
    L.bgr_aligner_configure.argtypes = [vp, u32, u32, u32]
    L.bgr_aligner_set_knob.argtypes = [vp, u32, u64]
    L.bgr_aligner_pass_counts.argtypes = [vp, vp]
    L.bgr_aligner_last_pass_runs.argtypes = [vp, C.POINTER(u32), C.POINTER(u32)]
    L.bgr_set_option.argtypes = [C.c_char_p, C.c_int64]
    L.bgr_get_option.argtypes = [C.c_char_p, C.POINTER(C.c_int64)]
    L.bgr_option_name.restype = C.c_char_p
    L.bgr_option_name.argtypes = [u32, C.POINTER(C.c_char_p)]
    L.bgr_plan_launch.argtypes = [C.POINTER(PlanInput), C.POINTER(PlanOutput)]
    L.bgr_readset_load.argtypes = [C.c_char_p, i32, u32, C.POINTER(vp)]
    L.bgr_readset_load_parallel.argtypes = [C.c_char_p, i32, u32, u32, u64, C.POINTER(vp)]
    L.bgr_align_all.argtypes = [vp, C.POINTER(Params), C.POINTER(RunOptions), C.c_char_p, C.c_char_p, C.c_char_p, vp, C.POINTER(C.c_double)]
    L.bgr_text_stage_device.argtypes = [vp]
    L.bgr_text_stage_upload_parts.argtypes = [vp, u32, vp, vp]
    L.bgr_device_alloc.argtypes = [i32, u64, C.POINTER(vp)]
    L.bgr_device_free.argtypes = [i32, vp]
    L.bgr_device_upload.argtypes = [i32, vp, vp, u64]
    L.bgr_device_download.argtypes = [i32, vp, vp, u64]
    L.bgr_host_alloc.argtypes = [u64, C.POINTER(vp)]
    L.bgr_host_free.argtypes = [vp]
    L.bgr_readset_count.restype = u64
    L.bgr_readset_count.argtypes = [vp]
    L.bgr_readset_view.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), C.POINTER(vp)]
    L.bgr_readset_destroy.argtypes = [vp]
    L.bgr_readset_destroy.restype = None
    L.bgr_write_records.argtypes = [vp, vp, u64, vp, vp, vp, vp, vp, vp]
    L.bgr_aligner_abundance_enable.argtypes = [vp, u32]
    L.bgr_aligner_abundance.argtypes = [vp, vp, u64]
    L.bgr_aligner_reset_abundance.argtypes = [vp]
    L.bgr_aligner_abundance_plan.argtypes = [vp, u64, u64, vp]
    L.bgr_plan_abundance.argtypes = [u64, u32, u64, u64, u32, u64, u32, vp]
    L.bgr_graph_abundance.argtypes = [vp, vp, u64]
    L.bgr_write_abundance.argtypes = [C.c_char_p, vp, vp, u64]
    L.bgr_aligner_links_enable.argtypes = [vp, u32]
    L.bgr_aligner_links.argtypes = [vp, vp, u64, vp]
    L.bgr_aligner_reset_links.argtypes = [vp]
    L.bgr_aligner_links_info.argtypes = [vp, vp]
    L.bgr_aligner_links_plan.argtypes = [vp, u64, vp]
    L.bgr_plan_links.argtypes = [u64, u64, u32, u32, vp]
    L.bgr_graph_links_bound.argtypes = [vp, vp]
    L.bgr_graph_links_enable.argtypes = [vp, u32]
    L.bgr_graph_links.argtypes = [vp, vp, u64, vp]
    L.bgr_write_gfa.argtypes = [C.c_char_p, vp, vp, u64, vp, u64]
    L.bgr_graph_links_enabled.argtypes = [vp]
    L.bgr_links_bubbles.argtypes = [C.c_int, vp, u64, u64, u64, vp, u64, vp]
    L.bgr_aligner_bubbles.argtypes = [vp, u64, vp, u64, vp]
    L.bgr_aligner_bubbles_times.argtypes = [vp, vp]
    L.bgr_graph_bubbles_enable.argtypes = [vp, u32, u64]
    L.bgr_graph_bubbles_enabled.argtypes = [vp]
    L.bgr_graph_bubbles.argtypes = [vp, vp, u64, vp]
    L.bgr_write_bubbles.argtypes = [C.c_char_p, vp, vp, u64]
    L.bgr_aligner_triples_enable.argtypes = [vp, u32]
    L.bgr_aligner_triples.argtypes = [vp, vp, u64, vp]
    L.bgr_aligner_reset_triples.argtypes = [vp]
    L.bgr_aligner_triples_info.argtypes = [vp, vp]
    L.bgr_triple_canonical.argtypes = [C.c_int32, C.c_int32, C.c_int32, vp]
    L.bgr_graph_triples_bound.argtypes = [vp, vp]
    L.bgr_graph_triples_enable.argtypes = [vp, u32]
    L.bgr_graph_triples_enabled.argtypes = [vp]
    L.bgr_graph_triples.argtypes = [vp, vp, u64, vp]
    L.bgr_write_triples.argtypes = [C.c_char_p, vp, vp, u64]
    L.bgr_bubbles_phase.argtypes = [vp, u64, vp, u64, vp, u64, vp]
    L.bgr_graph_phase_enable.argtypes = [vp, u32, u64]
    L.bgr_graph_phase_enabled.argtypes = [vp]
    L.bgr_graph_phase.argtypes = [vp, vp, u64, vp]
    L.bgr_write_phase.argtypes = [C.c_char_p, vp, vp, u64]
    L.bgr_phase_blocks.argtypes = [C.c_int, vp, u64, vp, u64, u64, u64, vp, u64, vp]
    L.bgr_phase_blocks_times.argtypes = [vp]
    L.bgr_graph_blocks_enable.argtypes = [vp, u32, u64, u64]
    L.bgr_graph_blocks_enabled.argtypes = [vp]
    L.bgr_graph_blocks.argtypes = [vp, vp, u64, vp]
    L.bgr_write_blocks.argtypes = [C.c_char_p, vp, vp, u64, vp, u64]
    L.bgr_blocks_haplotypes.argtypes = [vp, C.c_int, vp, u64, vp, u64, u64, vp, u64, vp, vp, u64, vp, vp]
    L.bgr_blocks_haplotypes_times.argtypes = [vp]
    L.bgr_graph_haplotypes_enable.argtypes = [vp, u32, u64, u64, u64]
    L.bgr_graph_haplotypes_enabled.argtypes = [vp]
    L.bgr_graph_haplotypes.argtypes = [vp, vp, u64, vp, vp, u64, vp]
    L.bgr_write_haplotypes.argtypes = [C.c_char_p, vp, vp, u64, vp, u64, vp, u64, vp, u64]
    L.bgr_graph_recompact.argtypes = [vp, C.c_int, vp, u64, vp, u64, vp, vp, u64, vp, vp, u64, vp]
    L.bgr_graph_recompact_times.argtypes = [vp]
    L.bgr_graph_recompact_enable.argtypes = [vp, u32, u64]
    L.bgr_graph_recompact_enabled.argtypes = [vp]
    L.bgr_graph_recompact_result.argtypes = [vp, vp, u64, vp, vp, u64, vp, vp, u64, vp]
    L.bgr_write_recompact.argtypes = [C.c_char_p, vp, vp, u64, vp, u64, vp, u64]
    L.bgr_blocks_tag_table.argtypes = [vp, u64, vp, u64, u64, u64, vp, vp]
    L.bgr_read_blocks_tags.argtypes = [C.c_char_p, u64, vp, vp]
    L.bgr_aligner_haplotag_enable.argtypes = [vp, vp, u64]
    L.bgr_aligner_haplotags.argtypes = [vp, u64, vp]
    L.bgr_graph_haplotag_enable.argtypes = [vp, vp, u64]
    L.bgr_graph_haplotag_enabled.argtypes = [vp]
    L.bgr_aligner_path_diffs.argtypes = [vp, vp, vp, u64, vp, vp, u64, vp]
    L.bgr_aligner_gaf_cs_enable.argtypes = [vp, C.c_int]
    L.bgr_graph_gaf_cs_enable.argtypes = [vp, C.c_int]
    L.bgr_graph_gaf_cs_enabled.argtypes = [vp]
    L.bgr_aligner_exhaustive_paths_enable.argtypes = [vp, C.c_int]
    L.bgr_aligner_device_rows_view.argtypes = [vp, C.POINTER(vp)]
    L.bgr_graph_exhaustive_paths_enable.argtypes = [vp, C.c_int]
    L.bgr_graph_exhaustive_paths_enabled.argtypes = [vp]
    L.bgr_graph_inside_build.argtypes = [vp]
    L.bgr_graph_inside_info.argtypes = [vp, C.POINTER(InsideInfo)]
    L.bgr_graph_inside_lookup.argtypes = [vp, C.c_uint64, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
    L.bgr_aligner_inside_enable.argtypes = [vp, C.c_int]
    L.bgr_aligner_inside_count.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.bgr_graph_inside_enable.argtypes = [vp, C.c_int]
    L.bgr_graph_inside_enabled.argtypes = [vp]
    L.bgr_graph_inside_count.argtypes = [vp, C.POINTER(C.c_uint64)]
    L.bgr_aligner_pileup_enable.argtypes = [vp, u32]
    L.bgr_aligner_pileup.argtypes = [vp, vp, u64, vp]
    L.bgr_aligner_reset_pileup.argtypes = [vp]
    L.bgr_graph_pileup_enable.argtypes = [vp, u32]
    L.bgr_graph_pileup_enabled.argtypes = [vp]
    L.bgr_graph_pileup.argtypes = [vp, vp, u64, vp]
    L.bgr_write_pileup.argtypes = [C.c_char_p, vp]
    L.bgr_aligner_pileup_sites.argtypes = [vp, vp, vp, u64, vp]
    L.bgr_aligner_pileup_sites_times.argtypes = [vp, vp]
    L.bgr_aligner_pileup_add.argtypes = [vp, vp]
    L.bgr_graph_variants_enable.argtypes = [vp, vp]
    L.bgr_graph_variants_enabled.argtypes = [vp]
    L.bgr_graph_variants.argtypes = [vp, vp, u64, vp]
    L.bgr_graph_variants_params.argtypes = [vp, vp]
    L.bgr_write_vcf.argtypes = [C.c_char_p, vp, vp, vp, u64]
    L.bgr_parse_af_ppm.argtypes = [C.c_char_p, vp]
    L.bgr_aligner_pileup_strands_enable.argtypes = [vp, u32]
    L.bgr_aligner_pileup_forward.argtypes = [vp, vp, u64]
    L.bgr_aligner_pileup_strand_sites.argtypes = [vp, vp, vp, u64, vp]
    L.bgr_graph_pileup_strands_enable.argtypes = [vp, u32]
    L.bgr_graph_pileup_strands_enabled.argtypes = [vp]
    L.bgr_graph_pileup_forward.argtypes = [vp, vp, u64]
    L.bgr_graph_variants_strands_enable.argtypes = [vp, vp]
    L.bgr_graph_variant_strand_sites.argtypes = [vp, vp, u64, vp]
    L.bgr_write_pileup_strands.argtypes = [C.c_char_p, vp]
    L.bgr_write_vcf_strands.argtypes = [C.c_char_p, vp, vp, vp, u64]
    L.bgr_parse_min_alt_strand.argtypes = [C.c_char_p, vp]
    L.bgr_write_depth.argtypes = [C.c_char_p, vp]
    L.bgr_link_canonical.argtypes = [C.c_int32, C.c_int32, vp, vp]
    _lib = L
    return L


def _check(rc):
    if rc != 0:
        raise BgrError("bgreat_gpu error %d: %s" % (rc, lib().bgr_last_error().decode("utf-8", "replace")))


def device_count():
    return lib().bgr_device_count()


def set_option(name, value):
    """Process-wide library option (bgr_set_option): the library reads no environment variables."""
    _check(lib().bgr_set_option(name.encode(), int(value)))


def get_option(name):
    v = C.c_int64(0)
    _check(lib().bgr_get_option(name.encode(), C.byref(v)))
    return int(v.value)


def option_names():
    out, i = [], 0
    while True:
        what = C.c_char_p()
        n = lib().bgr_option_name(i, C.byref(what))
        if n is None:
            return out
        out.append((n.decode(), what.value.decode()))
        i += 1


def set_options_from_string(spec):
    """"name=value,name=value" -> bgr_set_option (tools: their BGR_FUZZ_OPTIONS / --options; the LIBRARY reads no environment)."""
    for kv in filter(None, (spec or "").split(",")):
        k, v = kv.split("=")
        set_option(k.strip(), int(v))


class options:
    """with B.options(build_filter=2, **{"test.bases_cap": 5000}): ...  -- set, and put back on exit (tests)."""

    def __init__(self, **kv):
        self.kv, self.old = kv, {}

    def __enter__(self):
        for k, v in self.kv.items():
            self.old[k] = get_option(k)
            set_option(k, v)
        return self

    def __exit__(self, *exc):
        for k, v in self.old.items():
            set_option(k, v)
        return False


def plan_launch(**kw):
    """bgr_plan_launch: the launch geometry for a graph header / device / batch given as numbers (no device needed).  -> dict, or raises BgrError."""
    i, o = PlanInput(), PlanOutput()
    for k, v in kw.items():
        if k == "resident_waves":
            for j, w in enumerate(v):
                i.resident_waves[j] = int(w)
        else:
            setattr(i, k, int(v))
    _check(lib().bgr_plan_launch(C.byref(i), C.byref(o)))
    names = ["general", "greedy16", "exhaustive8", "anchors4", "depth_first_mid", "last"]
    d = {n: dict(used=bool(p.used), blocks=p.blocks, waves_per_block=p.waves_per_block, lds_bytes=p.lds_bytes, table_staged=bool(p.table_staged)) for n, p in zip(names, o.pass_)}
    d.update(level_search=bool(o.level_search), deep_only=bool(o.deep_only), x4_levels=o.x4_levels, memo_cap=o.memo_cap, deep_scratch_bytes=o.deep_scratch_bytes, arena_ints=o.arena_ints)
    return d


class DeviceBuffer:
    """A numpy array parked in a device's HBM through the C-ABI (bgr_device_alloc / upload): input of bgr_align_device."""

    def __init__(self, device, array):
        a = np.ascontiguousarray(array)
        self.device, self.nbytes = device, a.nbytes
        p = C.c_void_p()
        _check(lib().bgr_device_alloc(device, a.nbytes, C.byref(p)))
        self.ptr = p.value
        _check(lib().bgr_device_upload(device, self.ptr, a.ctypes.data, a.nbytes))

    def data_ptr(self):
        return self.ptr

    def free(self):
        if getattr(self, "ptr", None):
            lib().bgr_device_free(self.device, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:   # (interpreter shutdown: the library may be gone already)
            pass


def device_upload(device, ptr, array):
    """bgr_device_upload: the bytes of a numpy array -> device memory at ptr (the caller answers for the room there)."""
    a = np.ascontiguousarray(array)
    _check(lib().bgr_device_upload(device, ptr, a.ctypes.data, a.nbytes))


def device_download(device, ptr, count, dtype=np.uint8):
    """bgr_device_download: `count` items of `dtype` from device memory at ptr -> numpy array."""
    out = np.empty(count, dtype=dtype)
    _check(lib().bgr_device_download(device, out.ctypes.data, ptr, out.nbytes))
    return out


def _as_u8(a):
    if isinstance(a, (bytes, bytearray)):
        a = np.frombuffer(a, dtype=np.uint8)
    return np.ascontiguousarray(a, dtype=np.uint8)


def pack_reads(reads, offsets):
    """ASCII reads -> the 2-bit planes of bgr_align_batch_packed (host side; bgr_pack_reads).  -> dict of arrays."""
    reads = _as_u8(reads)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    n = len(offsets) - 1
    rel = offsets - offsets[0]
    total = int(rel[n])
    words = lib().bgr_packed_plane_words(n, total)
    fw3 = np.zeros(words, dtype=np.uint64)
    hasn = np.zeros((n + 31) // 32 + 1, dtype=np.uint32)
    cap = max(64, total // 16 + 64)
    nm_index = np.zeros(cap, dtype=np.uint32)
    nm_value = np.zeros(cap, dtype=np.uint64)
    cnt, mx = C.c_uint64(), C.c_uint32()
    _check(lib().bgr_pack_reads(reads.ctypes.data, offsets.ctypes.data, n, fw3.ctypes.data, hasn.ctypes.data, nm_index.ctypes.data,
                                nm_value.ctypes.data, cap, C.byref(cnt), C.byref(mx)))
    return {"read_offsets": rel, "fw3": fw3, "hasn": hasn, "nm_index": nm_index[: cnt.value].copy(), "nm_value": nm_value[: cnt.value].copy(),
            "max_read_len": mx.value, "n": n}


class Graph:
    """The immutable index (Aligner::indexUnitigs, aligner.cpp:407-547)."""

    def __init__(self, handle):
        self.h = handle

    @classmethod
    def build(cls, k, seqs, offsets, gamma=0.0, anchors=False, no_evictions=False):
        """anchors=True also builds the k-mer anchors index of -G mode (MODE_ANCHORS); gamma = key table slots per key (0 = default)."""
        seqs = _as_u8(seqs)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        h = C.c_void_p()
        _check(lib().bgr_graph_build_ex(k, len(offsets) - 1, seqs.ctypes.data, offsets.ctypes.data, gamma,
                                        (BUILD_ANCHORS if anchors else 0) | (BUILD_NO_EVICTIONS if no_evictions else 0), C.byref(h)))
        return cls(h)

    @classmethod
    def from_fasta(cls, path, k, gamma=0.0, anchors=False):
        h = C.c_void_p()
        _check(lib().bgr_graph_build_from_fasta_ex(path.encode(), k, gamma, BUILD_ANCHORS if anchors else 0, C.byref(h)))
        return cls(h)

    def key_lookup(self, key):
        """slot of a canonical (k-1)-mer (a non-negative int of up to 2(k-1) bits, any k) in the overlap key table, None for a non-member"""
        key = int(key)
        if key < 0:
            raise ValueError("key_lookup: a (k-1)-mer is a non-negative integer")
        if key >> 128:
            return None
        slot = C.c_uint32()
        _check(lib().bgr_graph_key_lookup_wide(self.h, key >> 64, key & 0xFFFFFFFFFFFFFFFF, C.byref(slot)))
        return None if slot.value == 0xFFFFFFFF else int(slot.value)

    def anchor_lookup(self, kmer):
        """(index, unitig, offset) of boomphf::mphf::lookup(kmer) on the anchors index; index None for ULLONG_MAX."""
        idx, pos = C.c_uint64(), C.c_uint64()
        _check(lib().bgr_graph_anchor_lookup(self.h, int(kmer), C.byref(idx), C.byref(pos)))
        if idx.value == 0xFFFFFFFFFFFFFFFF:
            return None, 0, 0
        return idx.value, pos.value >> 32, pos.value & 0xFFFFFFFF

    @classmethod
    def from_blob(cls, blob):
        blob = _as_u8(blob)
        h = C.c_void_p()
        _check(lib().bgr_graph_from_blob(blob.ctypes.data, blob.size, C.byref(h)))
        return cls(h)

    @classmethod
    def adopt_device_blob(cls, device, dev_ptr, nbytes):
        h = C.c_void_p()
        _check(lib().bgr_graph_adopt_device_blob(device, dev_ptr, nbytes, C.byref(h)))
        return cls(h)

    def blob(self):
        n = C.c_uint64()
        p = lib().bgr_graph_blob(self.h, C.byref(n))
        if not p:
            return np.zeros(0, dtype=np.uint8)
        v = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(n.value,)).view(_Borrowed)
        v._owner = self   # the bytes belong to the graph: keep it alive as long as the view (or a view of it) is
        return v

    def jump_index(self):
        """The jump index of the greedy anchor scan as uint32[buckets, 4] (two entries {id | flags, offset << 8 | tag} per bucket), or None.
        It is not part of blob()."""
        n = C.c_uint64()
        lib().bgr_graph_jump_index.restype = C.c_void_p
        lib().bgr_graph_jump_index.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        p = lib().bgr_graph_jump_index(self.h, C.byref(n))
        if not p:
            return None
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint32)), shape=(n.value // 16, 4)).copy()

    def info(self):
        gi = GraphInfo()
        _check(lib().bgr_graph_info(self.h, C.byref(gi)))
        return {f[0]: getattr(gi, f[0]) for f in GraphInfo._fields_ if f[0] != "reserved" and not f[0].startswith("jump_")}

    def jump_info(self):
        """The jump index of the greedy anchor scan (it lies behind the blob, so info() -- which describes the blob -- leaves it out): entries,
        bytes, sampling stride, drop rate x 1000, and why the graph has none (jump_absent: BGR_JUMP_*, jump_absent_why: in words, "" when it has one)."""
        gi = GraphInfo()
        _check(lib().bgr_graph_info(self.h, C.byref(gi)))
        d = {f[0]: getattr(gi, f[0]) for f in GraphInfo._fields_ if f[0].startswith("jump_")}
        d["jump_absent_why"] = JUMP_ABSENT[gi.jump_absent]
        return d

    def inside_build(self):
        """bgr_graph_inside_build: the inside index (an exact table over a sample of the unitigs' k-mers) on the host; sticky."""
        _check(lib().bgr_graph_inside_build(self.h))

    def inside_info(self):
        """bgr_graph_inside_info -> {entries, slots, bytes, build_seconds}; zeroes before inside_build()."""
        o = InsideInfo()
        _check(lib().bgr_graph_inside_info(self.h, C.byref(o)))
        return {f[0]: getattr(o, f[0]) for f in InsideInfo._fields_}

    def inside_lookup(self, kmer):
        """bgr_graph_inside_lookup: the entry of a k-mer word (either strand) -> (unitig id, offset, forward window is canonical), or None."""
        u, j, fc, found = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        _check(lib().bgr_graph_inside_lookup(self.h, int(kmer), C.byref(u), C.byref(j), C.byref(fc), C.byref(found)))
        return (int(u.value), int(j.value), bool(fc.value)) if found.value else None

    def inside_enable(self, on=True):
        """bgr_graph_inside_enable: sticky -- every aligner of a later align_all on this graph runs the inside pass."""
        _check(lib().bgr_graph_inside_enable(self.h, int(bool(on))))

    def inside_enabled(self):
        return bool(lib().bgr_graph_inside_enabled(self.h))

    def inside_count(self):
        """bgr_graph_inside_count: reads the last align_all with the switch on mapped inside a unitig."""
        n = C.c_uint64(0)
        _check(lib().bgr_graph_inside_count(self.h, C.byref(n)))
        return int(n.value)

    def upload(self, device=0):
        _check(lib().bgr_graph_upload(self.h, device))

    def devices_init(self, first_device=0, n_devices=1, how=0):
        """Graph resident on n devices: one upload, then RCCL broadcast / xGMI peer copies (bgr_devices_init) -> method used."""
        _check(lib().bgr_devices_init(self.h, first_device, n_devices, how))
        return lib().bgr_devices_method(self.h)

    def device_blob(self, device=0):
        return lib().bgr_graph_device_blob(self.h, device)

    def abundance(self):
        """bgr_graph_abundance: the per-unitig totals of the last align_all(..., abundance=True) on this graph -> uint64 (n_unitigs, 3) =
        (reads, bases, kmers), row i = unitig id i + 1.  Raises BgrError when there are none."""
        n = self.info()["n_unitigs"]
        out = np.zeros((n, 3), dtype=np.uint64)
        _check(lib().bgr_graph_abundance(self.h, out.ctypes.data, n))
        return out

    def links_enable(self, on=True):
        """bgr_graph_links_enable: sticky -- every later align_all on this graph counts unitig abundance and links."""
        _check(lib().bgr_graph_links_enable(self.h, int(bool(on))))

    def links_enabled(self):
        """bgr_graph_links_enabled: the switch as it stands."""
        return bool(lib().bgr_graph_links_enabled(self.h))

    def bubbles_enable(self, on=True, min_link=1):
        """bgr_graph_bubbles_enable: sticky -- every later align_all on this graph counts unitig abundance and links and calls the bubbles of the run's links."""
        _check(lib().bgr_graph_bubbles_enable(self.h, int(bool(on)), int(min_link)))

    def bubbles_enabled(self):
        """bgr_graph_bubbles_enabled: the switch as it stands."""
        return bool(lib().bgr_graph_bubbles_enabled(self.h))

    def bubbles(self):
        """bgr_graph_bubbles: the bubbles of the last align_all with the switch on -> array of BUBBLE_DTYPE, ordered by (|source|, source < 0)."""
        return _fetch_records(lambda out, cap, n: lib().bgr_graph_bubbles(self.h, out, cap, n), BUBBLE_DTYPE)

    def links(self):
        """bgr_graph_links: the links of the last align_all with the switch on -> array of LINK_DTYPE (from, to, count), canonical, sorted by key.
        Raises BgrError when there are none."""
        return _fetch_records(lambda out, cap, n: lib().bgr_graph_links(self.h, out, cap, n), LINK_DTYPE)

    def pileup_enable(self, on=True):
        """bgr_graph_pileup_enable: sticky -- every later align_all on this graph counts unitig abundance and the per-base pileup."""
        _check(lib().bgr_graph_pileup_enable(self.h, int(bool(on))))

    def pileup_enabled(self):
        """bgr_graph_pileup_enabled: the switch as it stands."""
        return bool(lib().bgr_graph_pileup_enabled(self.h))

    def pileup(self):
        """bgr_graph_pileup: the totals of the last align_all with the switch on -> (array of PILEUP_DTYPE (depth, a, c, g, t, n), one row per
        base, flat in unitig order; rows that spelled no walk).  Raises BgrError when there are none."""
        return _fetch_pileup(lib().bgr_graph_pileup, self)

    def write_pileup(self, path):
        """bgr_write_pileup: one line per position with a count."""
        _check(lib().bgr_write_pileup(path.encode(), self.h))

    def write_depth(self, path):
        """bgr_write_depth: one bedGraph-like line per run of equal non-zero depth."""
        _check(lib().bgr_write_depth(path.encode(), self.h))

    def variants_enable(self, min_depth=2, min_alt=2, min_af_ppm=200000, on=True):
        """bgr_graph_variants_enable: sticky -- every later align_all on this graph counts the pileup and calls SNV sites from it on the device
        (a base with depth >= min_depth where an allele has count >= min_alt and count * 1e6 >= min_af_ppm * depth).  on=False switches it off."""
        prm = VariantParams(int(min_depth), int(min_alt), int(min_af_ppm))
        _check(lib().bgr_graph_variants_enable(self.h, C.byref(prm) if on else None))

    def variants_enabled(self):
        """bgr_graph_variants_enabled: the switch as it stands."""
        return bool(lib().bgr_graph_variants_enabled(self.h))

    def variants(self):
        """bgr_graph_variants: the sites of the last align_all with the switch on -> array of VARIANT_DTYPE (unitig, pos, depth, a, c, g, t, n) in
        (unitig, pos) order.  Raises BgrError when there are none."""
        return _fetch_records(lambda out, cap, n: lib().bgr_graph_variants(self.h, out, cap, n), VARIANT_DTYPE)

    def variants_params(self):
        """bgr_graph_variants_params: (min_depth, min_alt, min_af_ppm) the sites of Graph.variants() were called with."""
        prm = VariantParams()
        _check(lib().bgr_graph_variants_params(self.h, C.byref(prm)))
        return int(prm.min_depth), int(prm.min_alt), int(prm.min_af_ppm)

    def write_vcf(self, path, sites=None, params=None):
        """bgr_write_vcf: `sites` (default: Graph.variants()) called with `params` (default: Graph.variants_params()) as VCF 4.2."""
        if sites is None:
            sites = self.variants()
        prm = VariantParams(*(self.variants_params() if params is None else params))
        sites = np.ascontiguousarray(sites, dtype=VARIANT_DTYPE)
        _check(lib().bgr_write_vcf(path.encode(), self.h, C.byref(prm), sites.ctypes.data if len(sites) else None, len(sites)))

    def pileup_strands_enable(self, on=True):
        """bgr_graph_pileup_strands_enable: sticky -- every later align_all also counts the forward pileup and gathers it next to the totals
        (switches pileup_enable on as well; on=False leaves that on)."""
        _check(lib().bgr_graph_pileup_strands_enable(self.h, int(bool(on))))

    def pileup_strands_enabled(self):
        """bgr_graph_pileup_strands_enabled: the switch as it stands."""
        return bool(lib().bgr_graph_pileup_strands_enabled(self.h))

    def pileup_forward(self):
        """bgr_graph_pileup_forward: the forward totals of the last align_all with the strands switch on -> array of PILEUP_DTYPE, one row per base."""
        return _fetch_forward(lib().bgr_graph_pileup_forward, self)

    def write_pileup_strands(self, path):
        """bgr_write_pileup_strands: write_pileup's lines with the six forward numbers appended."""
        _check(lib().bgr_write_pileup_strands(path.encode(), self.h))

    def variants_strands_enable(self, min_depth=2, min_alt=2, min_af_ppm=200000, min_alt_strand=0, on=True):
        """bgr_graph_variants_strands_enable: variants_enable with the strand filter -- an allele must also be read at least min_alt_strand times on
        each strand; the run keeps records of VARIANT_STRAND_DTYPE.  on=False switches the variants switch off."""
        prm = VariantStrandParams(int(min_depth), int(min_alt), int(min_af_ppm), int(min_alt_strand))
        _check(lib().bgr_graph_variants_strands_enable(self.h, C.byref(prm) if on else None))

    def variant_strand_sites(self):
        """bgr_graph_variant_strand_sites: the sites of the last align_all with variants_strands_enable on -> array of VARIANT_STRAND_DTYPE."""
        return _fetch_records(lambda out, cap, n: lib().bgr_graph_variant_strand_sites(self.h, out, cap, n), VARIANT_STRAND_DTYPE)

    def write_vcf_strands(self, path, sites, params):
        """bgr_write_vcf_strands: `sites` (VARIANT_STRAND_DTYPE) called with params = (min_depth, min_alt, min_af_ppm, min_alt_strand) as VCF 4.2 with ADF / ADR."""
        prm = VariantStrandParams(*(int(v) for v in params))
        sites = np.ascontiguousarray(sites, dtype=VARIANT_STRAND_DTYPE)
        _check(lib().bgr_write_vcf_strands(path.encode(), self.h, C.byref(prm), sites.ctypes.data if len(sites) else None, len(sites)))

    def triples_enable(self, on=True):
        """bgr_graph_triples_enable: sticky -- every later align_all on this graph counts unitig abundance and triples."""
        _check(lib().bgr_graph_triples_enable(self.h, int(bool(on))))

    def triples_enabled(self):
        """bgr_graph_triples_enabled: the switch as it stands."""
        return bool(lib().bgr_graph_triples_enabled(self.h))

    def triples(self):
        """bgr_graph_triples: the triples of the last align_all with the switch on -> array of TRIPLE_DTYPE, canonical, sorted by key."""
        return _fetch_records(lambda out, cap, n: lib().bgr_graph_triples(self.h, out, cap, n), TRIPLE_DTYPE)

    def triples_bound(self):
        """bgr_graph_triples_bound: how many distinct triples any rows on this graph can hold (the table of triples has at least twice as many slots)."""
        b = C.c_uint64(0)
        _check(lib().bgr_graph_triples_bound(self.h, C.byref(b)))
        return int(b.value)

    def phase_enable(self, on=True, min_link=1):
        """bgr_graph_phase_enable: sticky -- every later align_all on this graph counts links and triples, calls the bubbles and joins the neighbours."""
        _check(lib().bgr_graph_phase_enable(self.h, int(bool(on)), int(min_link)))

    def phase_enabled(self):
        """bgr_graph_phase_enabled: the switch as it stands."""
        return bool(lib().bgr_graph_phase_enabled(self.h))

    def phase(self):
        """bgr_graph_phase: the phase records of the last align_all with the switch on -> array of PHASE_DTYPE, ordered by via."""
        return _fetch_records(lambda out, cap, n: lib().bgr_graph_phase(self.h, out, cap, n), PHASE_DTYPE)

    def blocks_enable(self, on=True, min_link=1, min_phase=1):
        """bgr_graph_blocks_enable: sticky -- every later align_all on this graph does what phase_enable makes it do and chains the decided pairs into
        haplotype blocks on the device."""
        _check(lib().bgr_graph_blocks_enable(self.h, int(bool(on)), int(min_link), int(min_phase)))

    def blocks_enabled(self):
        """bgr_graph_blocks_enabled: the switch as it stands."""
        return bool(lib().bgr_graph_blocks_enabled(self.h))

    def blocks(self):
        """bgr_graph_blocks: the block entries of the last align_all with the switch on -> array of BLOCK_DTYPE, block after block in chain order."""
        return _fetch_records(lambda out, cap, n: lib().bgr_graph_blocks(self.h, out, cap, n), BLOCK_DTYPE)

    def haplotypes_enable(self, on=True, min_link=1, min_phase=1, min_block=1):
        """bgr_graph_haplotypes_enable: sticky -- every later align_all on this graph does what blocks_enable makes it do and spells the two sequences
        of every block of at least min_block bubbles on the device."""
        _check(lib().bgr_graph_haplotypes_enable(self.h, int(bool(on)), int(min_link), int(min_phase), int(min_block)))

    def haplotypes_enabled(self):
        """bgr_graph_haplotypes_enabled: the switch as it stands."""
        return bool(lib().bgr_graph_haplotypes_enabled(self.h))

    def haplotypes(self):
        """bgr_graph_haplotypes: the sequences of the last align_all with the switch on -> (array of HAPLOTYPE_DTYPE, block after block, A before B;
        the characters as one uint8 array the records point into)."""
        return _fetch_haplotypes(lambda out, cap, n, seq, seq_cap, seq_bytes: lib().bgr_graph_haplotypes(self.h, out, cap, n, seq, seq_cap, seq_bytes))

    def recompact(self, keep, device=0):
        """bgr_graph_recompact: the unitigs with a non-zero byte in `keep` (one per unitig 1..n) merged into maximal non-branching chains on `device`,
        where the graph must be resident -> (array of CHAIN_DTYPE in the reported order, the walks' oriented ids as one int32 array, the characters
        as one uint8 array).  The sizing call comes first."""
        keep = np.ascontiguousarray(keep, dtype=np.uint8)
        return _fetch_chains(lambda out, cap, n, walk, walk_cap, walk_n, seq, seq_cap, seq_bytes: lib().bgr_graph_recompact(
            self.h, int(device), keep.ctypes.data if len(keep) else None, keep.shape[0], out, cap, n, walk, walk_cap, walk_n, seq, seq_cap, seq_bytes))

    def recompact_enable(self, on=True, min_reads=1):
        """bgr_graph_recompact_enable: sticky -- every later align_all on this graph counts unitig abundance and, when it ends, compacts the unitigs
        with reads >= min_reads (0 keeps everything) on the device."""
        _check(lib().bgr_graph_recompact_enable(self.h, int(bool(on)), int(min_reads)))

    def recompact_enabled(self):
        """bgr_graph_recompact_enabled: the switch as it stands."""
        return bool(lib().bgr_graph_recompact_enabled(self.h))

    def recompact_result(self):
        """bgr_graph_recompact_result: the chains of the last align_all with the switch on -> (CHAIN_DTYPE records, int32 walk, uint8 characters)."""
        return _fetch_chains(lambda *a: lib().bgr_graph_recompact_result(self.h, *a))

    def haplotag_enable(self, table):
        """bgr_graph_haplotag_enable: sticky -- every later align_all with gaf on this graph tags its lines from `table` (n_unitigs + 1 uint32, as
        blocks_tag_table / read_blocks_tags make it; the graph keeps a copy); None switches it off."""
        if table is None:
            _check(lib().bgr_graph_haplotag_enable(self.h, None, 0))
            return
        table = np.ascontiguousarray(table, dtype=np.uint32)
        _check(lib().bgr_graph_haplotag_enable(self.h, table.ctypes.data, table.shape[0]))

    def haplotag_enabled(self):
        """bgr_graph_haplotag_enabled: the switch as it stands."""
        return bool(lib().bgr_graph_haplotag_enabled(self.h))

    def gaf_cs_enable(self, on=True):
        """bgr_graph_gaf_cs_enable: sticky -- the GAF lines of every later align_all with gaf on this graph end in the cs:Z: field."""
        _check(lib().bgr_graph_gaf_cs_enable(self.h, int(bool(on))))

    def gaf_cs_enabled(self):
        """bgr_graph_gaf_cs_enabled: the switch as it stands."""
        return bool(lib().bgr_graph_gaf_cs_enabled(self.h))

    def exhaustive_paths_enable(self, on=True):
        """bgr_graph_exhaustive_paths_enable: sticky -- a later align_all in exhaustive mode writes GAF lines (gaf) and counts what the graph's switches ask
        for, from the paths exhaustive mode finds (their end offset dropped)."""
        _check(lib().bgr_graph_exhaustive_paths_enable(self.h, int(bool(on))))

    def exhaustive_paths_enabled(self):
        """bgr_graph_exhaustive_paths_enabled: the switch as it stands."""
        return bool(lib().bgr_graph_exhaustive_paths_enabled(self.h))

    def links_bound(self):
        """bgr_graph_links_bound: how many distinct links any rows on this graph can hold (the table of links has at least twice as many slots)."""
        b = C.c_uint64(0)
        _check(lib().bgr_graph_links_bound(self.h, C.byref(b)))
        return int(b.value)

    def close(self):
        if self.h:
            lib().bgr_graph_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Aligner:
    """Batch form of alignReadGreedy / alignReadExhaustive on one GPU."""

    def __init__(self, graph, device=0):
        self.graph = graph
        self.h = C.c_void_p()
        _check(lib().bgr_aligner_create(graph.h, device, C.byref(self.h)))

    def configure(self, waves_per_block=0, blocks_per_cu=0, lds_mphf=0):
        _check(lib().bgr_aligner_configure(self.h, waves_per_block, blocks_per_cu, lds_mphf))

    def set_knob(self, knob, value):
        """Test / diagnostic hooks (KNOB_*), see include/bgreat_gpu.h."""
        _check(lib().bgr_aligner_set_knob(self.h, knob, int(value)))

    def align(self, reads, offsets, m=2, effort=2, mode=MODE_GREEDY, partial=False):
        """-> (paths int32[], path_offsets uint64[n+1], status uint8[n]) in input order."""
        reads = _as_u8(reads)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        cap = int(offsets[-1] - offsets[0]) + 8 * n + 8
        paths = np.empty(cap, dtype=np.int32)
        poffs = np.empty(n + 1, dtype=np.uint64)
        status = np.empty(max(n, 1), dtype=np.uint8)
        p = Params(mode, m, effort, int(partial))
        _check(lib().bgr_align_batch(self.h, C.byref(p), reads.ctypes.data, offsets.ctypes.data, n, paths.ctypes.data, cap,
                                     poffs.ctypes.data, status.ctypes.data))
        return paths[: int(poffs[n])].copy(), poffs, status[:n]

    def align_packed(self, pk, m=2, effort=2, mode=MODE_GREEDY, partial=False, out=None):
        """bgr_align_batch_packed on the dict pack_reads() returns -> (paths, path_offsets, status)."""
        n = pk["n"]
        cap = int(pk["read_offsets"][n]) + 8 * n + 8
        paths = np.empty(cap, dtype=np.int32)
        poffs = np.empty(n + 1, dtype=np.uint64)
        status = np.empty(max(n, 1), dtype=np.uint8)
        s = PackedReads(pk["read_offsets"].ctypes.data, pk["fw3"].ctypes.data, pk["hasn"].ctypes.data,
                        pk["nm_index"].ctypes.data if len(pk["nm_index"]) else None, pk["nm_value"].ctypes.data if len(pk["nm_value"]) else None,
                        len(pk["nm_index"]), pk["max_read_len"])
        p = Params(mode, m, effort, int(partial))
        _check(lib().bgr_align_batch_packed(self.h, C.byref(p), C.byref(s), n, paths.ctypes.data, cap, poffs.ctypes.data, status.ctypes.data))
        return paths[: int(poffs[n])].copy(), poffs, status[:n]

    def align_begin(self, reads, offsets, m=2, effort=2, mode=MODE_GREEDY, partial=False):
        """bgr_align_batch_begin: copy + launch enqueued, returns at once -> ticket (keeps the host arrays alive until align_wait)."""
        reads = _as_u8(reads)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        t = Ticket()
        p = Params(mode, m, effort, int(partial))
        _check(lib().bgr_align_batch_begin(self.h, C.byref(p), reads.ctypes.data, offsets.ctypes.data, len(offsets) - 1, C.byref(t)))
        return (t, reads, offsets)

    def align_test(self, ticket):
        rc = lib().bgr_align_batch_test(C.byref(ticket[0]))
        if rc < 0:
            _check(rc)
        return bool(rc)

    def align_wait(self, ticket):
        """bgr_align_batch_wait -> (paths, path_offsets, status) of the batch the ticket was given for."""
        t, reads, offsets = ticket
        n = len(offsets) - 1
        cap = int(offsets[-1] - offsets[0]) + 8 * n + 8
        paths = np.empty(cap, dtype=np.int32)
        poffs = np.empty(n + 1, dtype=np.uint64)
        status = np.empty(max(n, 1), dtype=np.uint8)
        _check(lib().bgr_align_batch_wait(C.byref(t), paths.ctypes.data, cap, poffs.ctypes.data, status.ctypes.data))
        return paths[: int(poffs[n])].copy(), poffs, status[:n]

    def align_fasta_text(self, text, m=2, effort=2, mode=MODE_GREEDY, partial=False, want_output=True, paths_cap=None, staged=False, fastq=False, parts=None, record_info=False):
        """bgr_align_fasta_text: a piece of a FASTA file (bytes) -> (paths bytes, notAligned bytes, info dict); info["irregular"] = the
        device left the piece to the host parser (nothing mapped).  want_output: 1 / True = the reference's records, 2 = corrected reads (-c), 3 = GAF
        lines (--gaf); info["no_walk"] is there (and "irregular" set) when a path of the piece spells no walk (2 and 3).  fastq: True / 1 = the piece is whole four-line FASTQ records instead, 2 = their
        header and read lines only.  A too small `paths_cap` is grown through bgr_aligner_fetch_text.  parts (with staged): byte offsets at which
        the piece is cut into host ranges sent with bgr_text_stage_upload_parts (the call itself then gets no host pointer)."""
        text = np.frombuffer(bytes(text), dtype=np.uint8) if not isinstance(text, np.ndarray) else _as_u8(text)
        n = len(text)
        pcap = n + 64 if paths_cap is None else paths_cap
        pout = np.empty(max(pcap, 1), dtype=np.uint8)
        nout = np.empty(n + 64, dtype=np.uint8)
        b = TextBatch(C.sizeof(TextBatch), text.ctypes.data if n else None, n, int(want_output), 0, pout.ctypes.data, pcap, nout.ctypes.data, n + 64, 0, 0, 0, 0, None)
        b.fastq = int(fastq)
        rinfo = None
        if record_info:
            rinfo = np.zeros(n // 24 + 1024, dtype=np.uint32)
            b.record_info_out, b.record_info_cap = rinfo.ctypes.data, len(rinfo)
        p = Params(mode, m, effort, int(partial))
        stage = C.c_void_p()
        if staged:  # the piece sent ahead on a copy stream of its own (bgr_text_stage_upload); the call orders itself behind it
            _check(lib().bgr_text_stage_create(0, C.byref(stage)))
            if parts is None:
                _check(lib().bgr_text_stage_upload(stage, text.ctypes.data if n else None, n))
            else:
                cuts = [0] + sorted(int(x) for x in parts) + [n]
                keep = [np.ascontiguousarray(text[cuts[i]: cuts[i + 1]]).copy() for i in range(len(cuts) - 1)]   # separate host ranges
                ptrs = (C.c_void_p * len(keep))(*[k.ctypes.data if len(k) else None for k in keep])
                lens = (C.c_uint64 * len(keep))(*[len(k) for k in keep])
                _check(lib().bgr_text_stage_upload_parts(stage, len(keep), ptrs, lens))
                b.text = None
            b.stage = stage
        try:
            rc = lib().bgr_align_fasta_text(self.h, C.byref(p), C.byref(b))
            if rc == -4:  # BGR_E_CAPACITY: the mapping is done, the bytes did not fit (the stage still holds the text the records are cut from)
                pout = np.empty(int(b.paths_bytes) + 64, dtype=np.uint8)
                b.paths_out, b.paths_cap = pout.ctypes.data, len(pout)
                rc = lib().bgr_aligner_fetch_text(self.h, C.byref(b))
        finally:
            if staged:
                lib().bgr_text_stage_destroy(stage)
        _check(rc)
        info = {"irregular": bool(b.irregular), "n_records": int(b.n_records), "n_accepted": int(b.n_accepted)}
        if b.irregular == 2:
            info["no_walk"] = True
        if rinfo is not None:  # one word per record: kept << 31 | mapped << 30 | read length
            info["records"] = rinfo[: int(b.n_records)].copy()
        return pout[: int(b.paths_bytes)].tobytes(), nout[: int(b.notaligned_bytes)].tobytes(), info

    def align_device(self, d_reads_ptr, d_offsets_ptr, n, total_bases, max_len, m=2, effort=2, mode=MODE_GREEDY, partial=False):
        p = Params(mode, m, effort, int(partial))
        _check(lib().bgr_align_device(self.h, C.byref(p), d_reads_ptr, d_offsets_ptr, n, total_bases, max_len))

    def fetch(self, n, cap):
        paths = np.empty(cap, dtype=np.int32)
        poffs = np.empty(n + 1, dtype=np.uint64)
        status = np.empty(max(n, 1), dtype=np.uint8)
        _check(lib().bgr_aligner_fetch(self.h, n, paths.ctypes.data, cap, poffs.ctypes.data, status.ctypes.data))
        return paths[: int(poffs[n])].copy(), poffs, status[:n]

    def device_results(self):
        """bgr_aligner_device_results -> (results, arena, cursor): the device pointers of the last launch's uint2 per read {arena index of its row,
        ints of the row | status << 24}, of the int32 arena the rows lie in and of the cursor block (valid until the next launch grows them)."""
        r, a, c = C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(lib().bgr_aligner_device_results(self.h, C.byref(r), C.byref(a), C.byref(c)))
        return r.value, a.value, c.value

    def arena_ints(self):
        """bgr_aligner_arena_ints: ints of the arena as the last launch planned it (the bound the counting kernels check a row against)."""
        n = C.c_uint64(0)
        _check(lib().bgr_aligner_arena_ints(self.h, C.byref(n)))
        return int(n.value)

    def path_stats(self, d_reads_ptr, d_offsets_ptr, n):
        """bgr_aligner_path_stats over the last align_device launch (the same device reads again) -> structured array of n rows with the fields
        path_len, path_start, aligned, mismatches (PATH_STAT_NO_WALK set there for a path that spells no walk; zeros for an unmapped read)."""
        out = np.zeros(n, dtype=np.dtype([("path_len", np.uint64), ("path_start", np.uint64), ("aligned", np.uint32), ("mismatches", np.uint32)]))
        assert out.dtype.itemsize == C.sizeof(PathStat)
        _check(lib().bgr_aligner_path_stats(self.h, d_reads_ptr, d_offsets_ptr, n, out.ctypes.data))
        return out

    def path_diffs(self, d_reads_ptr, d_offsets_ptr, n):
        """bgr_aligner_path_diffs over the last align_device launch (the same device reads again) -> (uint64 offsets, n + 1 of them; array of
        PATH_DIFF_DTYPE): the differences of read i are rows offsets[i] .. offsets[i + 1], ascending read_pos.  The two-call form: the count first."""
        assert PATH_DIFF_DTYPE.itemsize == 8
        offs, total = np.zeros(n + 1, dtype=np.uint64), C.c_uint64(0)
        rc = lib().bgr_aligner_path_diffs(self.h, d_reads_ptr, d_offsets_ptr, n, offs.ctypes.data, None, 0, C.byref(total))
        if rc != -4:   # (no difference at all, or an error that is not "there are *n of them")
            _check(rc)
            return offs, np.zeros(0, dtype=PATH_DIFF_DTYPE)
        out = np.zeros(total.value, dtype=PATH_DIFF_DTYPE)
        _check(lib().bgr_aligner_path_diffs(self.h, d_reads_ptr, d_offsets_ptr, n, offs.ctypes.data, out.ctypes.data, len(out), C.byref(total)))
        return offs, out

    def inside_enable(self, on=True):
        """bgr_aligner_inside_enable: every greedy / anchors launch is followed by the inside pass from now on (the graph needs inside_build())."""
        _check(lib().bgr_aligner_inside_enable(self.h, int(bool(on))))

    def inside_count(self):
        """bgr_aligner_inside_count: reads the inside pass has mapped on this aligner."""
        n = C.c_uint64(0)
        _check(lib().bgr_aligner_inside_count(self.h, C.byref(n)))
        return int(n.value)

    def gaf_cs_enable(self, on=True):
        """bgr_aligner_gaf_cs_enable: the GAF lines of align_fasta_text (want_output=3) end in the cs:Z: field from now on."""
        _check(lib().bgr_aligner_gaf_cs_enable(self.h, int(bool(on))))

    def exhaustive_paths_enable(self, on=True):
        """bgr_aligner_exhaustive_paths_enable: exhaustive launches are counted (abundance, links, triples, pileup) once they are settled, path_stats,
        path_diffs and haplotags accept an exhaustive last launch, and align_fasta_text writes GAF lines in exhaustive mode -- all through the view
        of the rows without their end offset."""
        _check(lib().bgr_aligner_exhaustive_paths_enable(self.h, int(bool(on))))

    def device_rows_view(self):
        """bgr_aligner_device_rows_view -> the device pointer of the view of the last (exhaustive) launch: uint2 per read, as device_results()' first
        pointer with every mapped row one int shorter (valid until the next launch)."""
        v = C.c_void_p()
        _check(lib().bgr_aligner_device_rows_view(self.h, C.byref(v)))
        return v.value

    def haplotag_enable(self, table):
        """bgr_aligner_haplotag_enable: `table` (n_unitigs + 1 uint32) onto the aligner's device -- haplotags() and the GAF lines of align_fasta_text
        are tagged from it; None switches it off and frees the copy."""
        if table is None:
            _check(lib().bgr_aligner_haplotag_enable(self.h, None, 0))
            return
        table = np.ascontiguousarray(table, dtype=np.uint32)
        _check(lib().bgr_aligner_haplotag_enable(self.h, table.ctypes.data, table.shape[0]))

    def haplotags(self, n):
        """bgr_aligner_haplotags over the rows of the last launch -> array of READ_TAG_DTYPE, n rows (zeros for an unmapped read)."""
        out = np.zeros(n, dtype=READ_TAG_DTYPE)
        _check(lib().bgr_aligner_haplotags(self.h, n, out.ctypes.data if n else None))
        return out

    def abundance_enable(self, on=True):
        """bgr_aligner_abundance_enable: every greedy / anchors launch from now on adds its rows to the aligner's per-unitig table."""
        _check(lib().bgr_aligner_abundance_enable(self.h, int(bool(on))))

    def abundance(self):
        """bgr_aligner_abundance -> uint64 (n_unitigs, 3) = (reads, bases, kmers) since enable / reset, row i = unitig id i + 1."""
        n = self.graph.info()["n_unitigs"]
        out = np.zeros((n, 3), dtype=np.uint64)
        assert C.sizeof(UnitigAbundance) == 24
        _check(lib().bgr_aligner_abundance(self.h, out.ctypes.data, n))
        return out

    def abundance_plan(self, n_reads, total_bases):
        """bgr_aligner_abundance_plan: the abundance kernel behind a launch of this size -> dict(form (1 = A, 2 = B), blocks, threads, lds_bytes)."""
        out = (C.c_uint32 * 4)()
        _check(lib().bgr_aligner_abundance_plan(self.h, int(n_reads), int(total_bases), out))
        return dict(zip(("form", "blocks", "threads", "lds_bytes"), (int(x) for x in out)))

    def reset_abundance(self):
        _check(lib().bgr_aligner_reset_abundance(self.h))

    def links_enable(self, on=True):
        """bgr_aligner_links_enable: every greedy / anchors launch from now on adds the consecutive pairs of its rows to the aligner's table of links."""
        _check(lib().bgr_aligner_links_enable(self.h, int(bool(on))))

    def links(self):
        """bgr_aligner_links -> array of LINK_DTYPE (from, to, count) since enable / reset: canonical links, sorted by key."""
        return _fetch_records(lambda out, cap, n: lib().bgr_aligner_links(self.h, out, cap, n), LINK_DTYPE)

    def bubbles(self, min_link=1):
        """bgr_aligner_bubbles: the bubbles of the aligner's table of links as it stands, called on the device -> array of BUBBLE_DTYPE, ordered by
        (|source|, source < 0)."""
        return _fetch_records(lambda out, cap, n: lib().bgr_aligner_bubbles(self.h, int(min_link), out, cap, n), BUBBLE_DTYPE)

    def bubbles_times(self):
        """bgr_aligner_bubbles_times -> the last bubbles() call's four launches in milliseconds (adjacency, count, scan, emit)."""
        out = (C.c_double * 4)()
        _check(lib().bgr_aligner_bubbles_times(self.h, out))
        return [float(x) for x in out]

    def links_info(self):
        """bgr_aligner_links_info -> dict(capacity, bound, overflow, lds_fell_through)."""
        out = (C.c_uint64 * 4)()
        _check(lib().bgr_aligner_links_info(self.h, out))
        return dict(zip(("capacity", "bound", "overflow", "lds_fell_through"), (int(x) for x in out)))

    def links_plan(self, n_reads):
        """bgr_aligner_links_plan: the links kernel behind a launch of this size -> dict(form (1 = A, 2 = B), blocks, threads, lds_bytes)."""
        out = (C.c_uint32 * 4)()
        _check(lib().bgr_aligner_links_plan(self.h, int(n_reads), out))
        return dict(zip(("form", "blocks", "threads", "lds_bytes"), (int(x) for x in out)))

    def reset_links(self):
        _check(lib().bgr_aligner_reset_links(self.h))

    def triples_enable(self, on=True):
        """bgr_aligner_triples_enable: every greedy / anchors launch from now on adds every three consecutive ids of its rows to the aligner's table of triples."""
        _check(lib().bgr_aligner_triples_enable(self.h, int(bool(on))))

    def triples(self):
        """bgr_aligner_triples -> array of TRIPLE_DTYPE (from, via, to, reserved, count) since enable / reset: canonical triples, sorted by key."""
        return _fetch_records(lambda out, cap, n: lib().bgr_aligner_triples(self.h, out, cap, n), TRIPLE_DTYPE)

    def triples_info(self):
        """bgr_aligner_triples_info -> dict(capacity, bound, overflow, used)."""
        out = (C.c_uint64 * 4)()
        _check(lib().bgr_aligner_triples_info(self.h, out))
        return dict(capacity=int(out[0]), bound=int(out[1]), overflow=int(out[2]), used=int(out[3]))

    def reset_triples(self):
        _check(lib().bgr_aligner_reset_triples(self.h))

    def pileup_enable(self, on=True):
        """bgr_aligner_pileup_enable: every greedy / anchors launch from now on adds per-base depth and mismatches to the aligner's table
        (and its rows to the abundance table, which guards the depths)."""
        _check(lib().bgr_aligner_pileup_enable(self.h, int(bool(on))))

    def pileup(self):
        """bgr_aligner_pileup -> (array of PILEUP_DTYPE (depth, a, c, g, t, n) since enable / reset, one row per base, flat in unitig order;
        rows that spelled no walk)."""
        return _fetch_pileup(lib().bgr_aligner_pileup, self)

    def reset_pileup(self):
        _check(lib().bgr_aligner_reset_pileup(self.h))

    def pileup_sites(self, min_depth=2, min_alt=2, min_af_ppm=200000):
        """bgr_aligner_pileup_sites -> array of VARIANT_DTYPE: the SNV sites of this aligner's pileup table, called on the device (five launches
        on the aligner's stream); only the records cross to the host."""
        prm = VariantParams(int(min_depth), int(min_alt), int(min_af_ppm))
        return _fetch_records(lambda out, cap, n: lib().bgr_aligner_pileup_sites(self.h, C.byref(prm), out, cap, n), VARIANT_DTYPE)

    def pileup_strands_enable(self, on=True):
        """bgr_aligner_pileup_strands_enable: the pileup kernel of every launch from now on also adds the forward observations to a second table
        (enables the pileup as well; on=False keeps the table and leaves the pileup on)."""
        _check(lib().bgr_aligner_pileup_strands_enable(self.h, int(bool(on))))

    def pileup_forward(self):
        """bgr_aligner_pileup_forward -> array of PILEUP_DTYPE: the forward pileup since enable / reset, one row per base, flat in unitig order."""
        return _fetch_forward(lib().bgr_aligner_pileup_forward, self)

    def pileup_strand_sites(self, min_depth=2, min_alt=2, min_af_ppm=200000, min_alt_strand=0):
        """bgr_aligner_pileup_strand_sites -> array of VARIANT_STRAND_DTYPE: pileup_sites under the strand filter, with the forward numbers."""
        prm = VariantStrandParams(int(min_depth), int(min_alt), int(min_af_ppm), int(min_alt_strand))
        return _fetch_records(lambda out, cap, n: lib().bgr_aligner_pileup_strand_sites(self.h, C.byref(prm), out, cap, n), VARIANT_STRAND_DTYPE)

    def pileup_sites_times(self):
        """bgr_aligner_pileup_sites_times -> the milliseconds of the last pileup_sites' five launches (tile sums, scan, classify, scan, emit)."""
        ms = (C.c_double * 5)()
        _check(lib().bgr_aligner_pileup_sites_times(self.h, ms))
        return [float(x) for x in ms]

    def pileup_add(self, other):
        """bgr_aligner_pileup_add: other's pileup table is added into this aligner's, on the device(s); the abundance tables are not touched."""
        _check(lib().bgr_aligner_pileup_add(self.h, other.h))

    def sync(self):
        _check(lib().bgr_aligner_sync(self.h))

    def counters(self):
        out = np.zeros(5, dtype=np.uint64)
        _check(lib().bgr_aligner_counters(self.h, out.ctypes.data))
        return dict(zip(["reads", "no_overlap", "aligned", "not_aligned", "overlaps"], (int(x) for x in out)))

    def reset_counters(self):
        _check(lib().bgr_aligner_reset_counters(self.h))

    def kernel_time(self):
        n, ms = C.c_uint64(), C.c_double()
        _check(lib().bgr_aligner_kernel_time(self.h, C.byref(n), C.byref(ms)))
        return n.value, ms.value

    def kernel_times(self):
        """-> (launches, [(kernel name, summed ms), ...]) per kernel of a launch, in launch order."""
        n = C.c_uint64()
        ms = (C.c_double * 8)()
        names = (C.c_char_p * 8)()
        _check(lib().bgr_aligner_kernel_times(self.h, C.byref(n), ms, names))
        return n.value, [(names[i].decode(), ms[i]) for i in range(8) if names[i]]

    def reset_kernel_time(self):
        _check(lib().bgr_aligner_reset_kernel_time(self.h))

    def launch_info(self):
        out = np.zeros(4, dtype=np.uint32)
        _check(lib().bgr_aligner_launch_info(self.h, out.ctypes.data))
        return {"blocks": int(out[0]), "threads": int(out[1]), "lds_bytes": int(out[2]), "mphf_in_lds": bool(out[3] & 1),
                "level_search": bool(out[3] & 2), "four_reads_per_wave": bool(out[3] & 4)}

    def pass_counts(self):
        """Reads each pass of the last launch handed on (see bgr_aligner_pass_counts): 4 ints."""
        out = np.zeros(4, dtype=np.uint32)
        _check(lib().bgr_aligner_pass_counts(self.h, out.ctypes.data))
        return tuple(int(x) for x in out)

    def last_pass_runs(self):
        """Exhaustive mode: (runs of the last pass for the launch last settled, entries per wave of its table of remembered calls in the final run)."""
        r, c = C.c_uint32(0), C.c_uint32(0)
        _check(lib().bgr_aligner_last_pass_runs(self.h, C.byref(r), C.byref(c)))
        return int(r.value), int(c.value)

    def close(self):
        if self.h:
            lib().bgr_aligner_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def align_all(graph, reads_csv, paths_file, notaligned_file, m=2, effort=2, mode=MODE_GREEDY, partial=False, n_gpus=1, threads=1,
              batch_reads=0, chunk_bytes=0, fastq=False, write_exhaustive=False, correction=False, no_overlap_file=None, first_device=0, route=0, numa=0, split_output=False,
              gaf=False, abundance=False, links=None, pileup=None, exhaustive_paths=None):
    """Aligner::alignAll (aligner.cpp:550-597) as one call -> (counters dict, mapping seconds).  route: 0 = FASTA goes through the device as
    text when it can (bgr_align_fasta_text), 1 = host parser + host formatter always.  split_output: one pipeline per device, device d
    writing `<paths_file>.<d>` / `<notaligned_file>.<d>` (their concatenation = the single-file bytes).  gaf: the paths file holds one GAF line per
    mapped read instead of header + path ints (bgr_run_options.gaf: greedy modes, ACGT-only unitigs, not with correction).  abundance: count per unitig the reads, bases and k-mers mapped onto it
    (bgr_run_options.abundance; greedy modes); Graph.abundance() then has the run's totals.  links: True / False sets the graph's switch (Graph.links_enable) for this call and puts it back
    afterwards -- the run counts unitig abundance and links, Graph.abundance() and Graph.links() then have its totals; None leaves the switch as it is.
    pileup: likewise the graph's pileup switch (Graph.pileup_enable); Graph.pileup() then has the run's per-base totals.
    exhaustive_paths: likewise the graph's switch of the same name (Graph.exhaustive_paths_enable): a run in exhaustive mode then takes gaf and the counting switches."""
    if exhaustive_paths is not None:
        before = graph.exhaustive_paths_enabled()
        graph.exhaustive_paths_enable(exhaustive_paths)
        try:
            return align_all(graph, reads_csv, paths_file, notaligned_file, m, effort, mode, partial, n_gpus, threads, batch_reads, chunk_bytes, fastq, write_exhaustive,
                             correction, no_overlap_file, first_device, route, numa, split_output, gaf, abundance, links, pileup)
        finally:
            graph.exhaustive_paths_enable(before)
    if pileup is not None:
        before = graph.pileup_enabled()
        graph.pileup_enable(pileup)
        try:
            return align_all(graph, reads_csv, paths_file, notaligned_file, m, effort, mode, partial, n_gpus, threads, batch_reads, chunk_bytes, fastq, write_exhaustive,
                             correction, no_overlap_file, first_device, route, numa, split_output, gaf, abundance, links)
        finally:
            graph.pileup_enable(before)
    if links is not None:
        before = graph.links_enabled()
        graph.links_enable(links)
        try:
            return align_all(graph, reads_csv, paths_file, notaligned_file, m, effort, mode, partial, n_gpus, threads, batch_reads, chunk_bytes, fastq, write_exhaustive,
                             correction, no_overlap_file, first_device, route, numa, split_output, gaf, abundance)
        finally:
            graph.links_enable(before)
    p = Params(mode, m, effort, int(partial))
    o = RunOptions(C.sizeof(RunOptions), n_gpus, threads, batch_reads, chunk_bytes, int(fastq), int(write_exhaustive), 0, int(correction),
                   no_overlap_file.encode() if no_overlap_file else None, first_device, route, numa, int(split_output), int(gaf), int(abundance))
    out = np.zeros(5, dtype=np.uint64)
    secs = C.c_double()
    _check(lib().bgr_align_all(graph.h, C.byref(p), C.byref(o), reads_csv.encode(), paths_file.encode(), notaligned_file.encode(),
                               out.ctypes.data, C.byref(secs)))
    return dict(zip(["reads", "no_overlap", "aligned", "not_aligned", "overlaps"], (int(x) for x in out))), secs.value


def plan_abundance(n_unitigs, k, n_reads, total_bases, num_cus=0, lds_per_cu=0, form=0):
    """bgr_plan_abundance: the choice between the abundance kernel's forms from plain numbers (no device) -> dict as Aligner.abundance_plan."""
    out = (C.c_uint32 * 4)()
    _check(lib().bgr_plan_abundance(int(n_unitigs), int(k), int(n_reads), int(total_bases), int(num_cus), int(lds_per_cu), int(form), out))
    return dict(zip(("form", "blocks", "threads", "lds_bytes"), (int(x) for x in out)))


PILEUP_DTYPE = np.dtype([("depth", np.uint32), ("a", np.uint32), ("c", np.uint32), ("g", np.uint32), ("t", np.uint32), ("n", np.uint32)])


VARIANT_DTYPE = np.dtype([(f, np.uint32) for f in ("unitig", "pos", "depth", "a", "c", "g", "t", "n")])   # an array of bgr_variant_site
VARIANTS_TILE = 2048   # BGR_VARIANTS_TILE: words of the difference array per tile of the passes


class VariantParams(C.Structure):  # bgr_variant_params
    _fields_ = [("min_depth", C.c_uint32), ("min_alt", C.c_uint32), ("min_af_ppm", C.c_uint32)]


# an array of bgr_variant_strand_site: the numbers of bgr_variant_site, those of the forward table, two reserved words
VARIANT_STRAND_DTYPE = np.dtype([(f, np.uint32) for f in ("unitig", "pos", "depth", "a", "c", "g", "t", "n", "fdepth", "fa", "fc", "fg", "ft", "fn", "reserved0", "reserved1")])


class VariantStrandParams(C.Structure):  # bgr_variant_strand_params
    _fields_ = [("min_depth", C.c_uint32), ("min_alt", C.c_uint32), ("min_af_ppm", C.c_uint32), ("min_alt_strand", C.c_uint32)]


def _fetch_forward(fn, obj):
    g = obj if isinstance(obj, Graph) else obj.graph
    n = g.info()["total_bases"] // 2
    out = np.zeros(n, dtype=PILEUP_DTYPE)
    _check(fn(obj.h, out.ctypes.data, n))
    return out


def parse_min_alt_strand(text):
    """bgr_parse_min_alt_strand: the CLI's --min-alt-strand parser; BgrError for anything but at most nine digits."""
    v = C.c_uint32(0)
    _check(lib().bgr_parse_min_alt_strand(text.encode(), C.byref(v)))
    return int(v.value)


def parse_af_ppm(text):
    """bgr_parse_af_ppm: the CLI's --min-af parser -> parts per million; BgrError for anything but a decimal in 0 .. 1 with at most six places."""
    ppm = C.c_uint32(0)
    _check(lib().bgr_parse_af_ppm(text.encode(), C.byref(ppm)))
    return int(ppm.value)


def _fetch_pileup(fn, obj):
    g = obj if isinstance(obj, Graph) else obj.graph
    n = g.info()["total_bases"] // 2
    out = np.zeros(n, dtype=PILEUP_DTYPE)
    skipped = C.c_uint64(0)
    _check(fn(obj.h, out.ctypes.data, n, C.byref(skipped)))
    return out, int(skipped.value)


def _fetch_records(call, dtype):
    """the two-call form of the calls that deliver records (links, bubbles, triples, phase records, block entries, sites): the number first
    (BGR_E_CAPACITY with it), then the records"""
    assert LINK_DTYPE.itemsize == C.sizeof(Link) == 16 and BUBBLE_DTYPE.itemsize == C.sizeof(Bubble) == 48
    assert TRIPLE_DTYPE.itemsize == C.sizeof(Triple) == 24 and PHASE_DTYPE.itemsize == C.sizeof(Phase) == 64
    n = C.c_uint64(0)
    rc = call(None, 0, C.byref(n))
    if rc != -4 or n.value == 0:   # (no records, or an error that is not "there are n of them": an overflowed table is BGR_E_CAPACITY with n = 0, and says so)
        _check(rc)
        return np.zeros(0, dtype=dtype)
    out = np.zeros(n.value, dtype=dtype)
    _check(call(out.ctypes.data, n.value, C.byref(n)))
    return out[: n.value]


def _as_triples(triples):
    if not (isinstance(triples, np.ndarray) and triples.dtype == TRIPLE_DTYPE):
        triples = np.array([(int(a), int(b), int(c), 0, int(n)) for a, b, c, n in triples], dtype=TRIPLE_DTYPE)
    return np.ascontiguousarray(triples)


def triple_canonical(a, b, c):
    """bgr_triple_canonical: the canonical form of the triple (a, b, c), by the code the kernel runs -> (from, via, to)."""
    out = Triple()
    _check(lib().bgr_triple_canonical(int(a), int(b), int(c), C.byref(out)))
    return int(out.from_), int(out.via), int(out.to)


def write_triples(path, graph, triples):
    """bgr_write_triples: `triples` (an array of TRIPLE_DTYPE, or (from, via, to, count) tuples; sorted by key as Graph.triples() delivers them) as
    text -- "#from via to count", one tab-separated line per triple."""
    triples = _as_triples(triples)
    _check(lib().bgr_write_triples(path.encode(), graph.h, triples.ctypes.data if len(triples) else None, triples.shape[0]))


def bubbles_phase(bubbles, triples):
    """bgr_bubbles_phase: the neighbour pairs of `bubbles` (an array of BUBBLE_DTYPE, as Graph.bubbles() delivers them) with the counts of the
    triples (TRIPLE_DTYPE or (from, via, to, count) tuples; canonical, sorted) that thread them -> array of PHASE_DTYPE, ordered by via."""
    bubbles = np.ascontiguousarray(bubbles, dtype=BUBBLE_DTYPE)
    triples = _as_triples(triples)
    return _fetch_records(lambda out, cap, n: lib().bgr_bubbles_phase(bubbles.ctypes.data if len(bubbles) else None, bubbles.shape[0],
                                                                      triples.ctypes.data if len(triples) else None, triples.shape[0], out, cap, n), PHASE_DTYPE)


def write_phase(path, graph, records):
    """bgr_write_phase: `records` (an array of PHASE_DTYPE) as text -- "#via source in1 in2 out1 out2 sink n11 n12 n21 n22 phase", one tab-separated
    line per record."""
    records = np.ascontiguousarray(records, dtype=PHASE_DTYPE)
    _check(lib().bgr_write_phase(path.encode(), graph.h, records.ctypes.data if len(records) else None, records.shape[0]))


def phase_blocks(bubbles, phase, n_unitigs, min_phase=1, device=0):
    """bgr_phase_blocks: `bubbles` (an array of BUBBLE_DTYPE, as Graph.bubbles() delivers them) and the phase records made from them (PHASE_DTYPE, as
    bubbles_phase delivers them) chained into haplotype blocks on `device` -> array of BLOCK_DTYPE, one entry per bubble."""
    assert BLOCK_DTYPE.itemsize == C.sizeof(BlockEntry) == 24
    bubbles = np.ascontiguousarray(bubbles, dtype=BUBBLE_DTYPE)
    phase = np.ascontiguousarray(phase, dtype=PHASE_DTYPE)
    return _fetch_records(lambda out, cap, n: lib().bgr_phase_blocks(int(device), bubbles.ctypes.data if len(bubbles) else None, bubbles.shape[0], phase.ctypes.data if len(phase) else None,
                                                                     phase.shape[0], int(n_unitigs), int(min_phase), out, cap, n), BLOCK_DTYPE)


def phase_blocks_times():
    """bgr_phase_blocks_times: milliseconds of this thread's last phase_blocks -> dict(link, rank, place, total)."""
    ms = (C.c_double * 4)()
    _check(lib().bgr_phase_blocks_times(ms))
    return dict(zip(("link", "rank", "place", "total"), (float(x) for x in ms)))


def write_blocks(path, graph, bubbles, entries):
    """bgr_write_blocks: `entries` (an array of BLOCK_DTYPE) over `bubbles` (BUBBLE_DTYPE) as text -- "#block index size bubble source sink hapA hapB
    strand ring", one tab-separated line per entry."""
    bubbles = np.ascontiguousarray(bubbles, dtype=BUBBLE_DTYPE)
    entries = np.ascontiguousarray(entries, dtype=BLOCK_DTYPE)
    _check(lib().bgr_write_blocks(path.encode(), graph.h, bubbles.ctypes.data if len(bubbles) else None, bubbles.shape[0], entries.ctypes.data if len(entries) else None, entries.shape[0]))


READ_TAG_DTYPE = np.dtype([("block", np.uint32), ("a", np.uint32), ("b", np.uint32), ("others", np.uint32)])   # an array of bgr_read_tag


def blocks_tag_table(bubbles, entries, n_unitigs, min_block=1):
    """bgr_blocks_tag_table: the tag table of the blocks of at least min_block bubbles, from `bubbles` (BUBBLE_DTYPE) and `entries` (BLOCK_DTYPE)
    -> (uint32 array of n_unitigs + 1: block << 1 | hap per branch unitig, else 0; the number of tagged unitigs)."""
    bubbles = np.ascontiguousarray(bubbles, dtype=BUBBLE_DTYPE)
    entries = np.ascontiguousarray(entries, dtype=BLOCK_DTYPE)
    table, n = np.zeros(int(n_unitigs) + 1, dtype=np.uint32), C.c_uint64(0)
    _check(lib().bgr_blocks_tag_table(bubbles.ctypes.data if len(bubbles) else None, bubbles.shape[0], entries.ctypes.data if len(entries) else None, entries.shape[0], int(n_unitigs),
                                      int(min_block), table.ctypes.data, C.byref(n)))
    return table, int(n.value)


def read_blocks_tags(path, n_unitigs):
    """bgr_read_blocks_tags: the tag table from a --blocks file (every block of it tags) -> (uint32 array of n_unitigs + 1, the number of tagged unitigs)."""
    table, n = np.zeros(int(n_unitigs) + 1, dtype=np.uint32), C.c_uint64(0)
    _check(lib().bgr_read_blocks_tags(str(path).encode(), int(n_unitigs), table.ctypes.data, C.byref(n)))
    return table, int(n.value)


def _fetch_haplotypes(call):
    """the two-call form with two buffers: both sizes first (BGR_E_CAPACITY with them), then the records and the characters"""
    assert HAPLOTYPE_DTYPE.itemsize == C.sizeof(Haplotype) == 32
    n, nb = C.c_uint64(0), C.c_uint64(0)
    rc = call(None, 0, C.byref(n), None, 0, C.byref(nb))
    if rc != -4 or n.value == 0:   # (no sequences, or an error that is not "there are n of them")
        _check(rc)
        return np.zeros(0, dtype=HAPLOTYPE_DTYPE), np.zeros(0, dtype=np.uint8)
    out, seq = np.zeros(n.value, dtype=HAPLOTYPE_DTYPE), np.zeros(nb.value, dtype=np.uint8)
    _check(call(out.ctypes.data, n.value, C.byref(n), seq.ctypes.data if nb.value else None, nb.value, C.byref(nb)))
    return out[: n.value], seq[: nb.value]


def _fetch_chains(call):
    """the two-call form with three buffers: the sizes first (BGR_E_CAPACITY with them), then the records, the walk and the characters"""
    n, nw, nb = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    rc = call(None, 0, C.byref(n), None, 0, C.byref(nw), None, 0, C.byref(nb))
    if rc != -4 or n.value == 0:   # (no chains, or an error that is not "there are n of them")
        _check(rc)
        return np.zeros(0, dtype=CHAIN_DTYPE), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.uint8)
    out, walk, seq = np.zeros(n.value, dtype=CHAIN_DTYPE), np.zeros(nw.value, dtype=np.int32), np.zeros(nb.value, dtype=np.uint8)
    _check(call(out.ctypes.data, n.value, C.byref(n), walk.ctypes.data, nw.value, C.byref(nw), seq.ctypes.data, nb.value, C.byref(nb)))
    return out[: n.value], walk[: nw.value], seq[: nb.value]


def recompact_times():
    """bgr_graph_recompact_times: milliseconds of this thread's last Graph.recompact -> dict(links, rank, place, spell, records)."""
    ms = (C.c_double * 5)()
    _check(lib().bgr_graph_recompact_times(ms))
    return dict(zip(("links", "rank", "place", "spell", "records"), (float(x) for x in ms)))


def write_recompact(path, graph, records, walk, seq):
    """bgr_write_recompact: per chain the line ">{ordinal} LN:i:{length} unitigs={m} ring={.|circular} walk={>12<7>9}" and the sequence on one line: a
    unitig file that Graph.from_fasta / bgreat -g reads."""
    records = np.ascontiguousarray(records, dtype=CHAIN_DTYPE)
    walk = np.ascontiguousarray(walk, dtype=np.int32)
    seq = np.ascontiguousarray(seq, dtype=np.uint8)
    _check(lib().bgr_write_recompact(path.encode(), graph.h, records.ctypes.data if len(records) else None, records.shape[0], walk.ctypes.data if len(walk) else None, walk.shape[0],
                                     seq.ctypes.data if len(seq) else None, seq.shape[0]))


def blocks_haplotypes(graph, bubbles, entries, min_block=1, device=0):
    """bgr_blocks_haplotypes: the two sequences of every block of at least min_block bubbles, spelled on `device` (where `graph` must be resident) from
    `bubbles` (BUBBLE_DTYPE, as Graph.bubbles() delivers them) and `entries` (BLOCK_DTYPE, as phase_blocks / Graph.blocks() deliver them for these
    bubbles) -> (array of HAPLOTYPE_DTYPE, the characters as one uint8 array, the number of bad junctions)."""
    bubbles = np.ascontiguousarray(bubbles, dtype=BUBBLE_DTYPE)
    entries = np.ascontiguousarray(entries, dtype=BLOCK_DTYPE)
    bad = C.c_uint64(0)
    recs, seq = _fetch_haplotypes(lambda out, cap, n, sq, seq_cap, seq_bytes: lib().bgr_blocks_haplotypes(
        graph.h, int(device), bubbles.ctypes.data if len(bubbles) else None, bubbles.shape[0], entries.ctypes.data if len(entries) else None, entries.shape[0], int(min_block), out, cap, n, sq,
        seq_cap, seq_bytes, C.byref(bad)))
    return recs, seq, int(bad.value)


def blocks_haplotypes_times():
    """bgr_blocks_haplotypes_times: milliseconds of this thread's last blocks_haplotypes -> dict(items, spell, records, total)."""
    ms = (C.c_double * 4)()
    _check(lib().bgr_blocks_haplotypes_times(ms))
    return dict(zip(("items", "spell", "records", "total"), (float(x) for x in ms)))


def write_haplotypes(path, graph, bubbles, entries, records, seq):
    """bgr_write_haplotypes: per record the line ">block<b>_<A|B> bubbles=<size> length=<L> ring=<.|circular|conflict> walk=<w>" and the sequence on one
    line; the walk (GAF notation) is built from `entries` (BLOCK_DTYPE) over `bubbles` (BUBBLE_DTYPE)."""
    bubbles = np.ascontiguousarray(bubbles, dtype=BUBBLE_DTYPE)
    entries = np.ascontiguousarray(entries, dtype=BLOCK_DTYPE)
    records = np.ascontiguousarray(records, dtype=HAPLOTYPE_DTYPE)
    seq = np.ascontiguousarray(seq, dtype=np.uint8)
    _check(lib().bgr_write_haplotypes(path.encode(), graph.h, bubbles.ctypes.data if len(bubbles) else None, bubbles.shape[0], entries.ctypes.data if len(entries) else None, entries.shape[0],
                                      records.ctypes.data if len(records) else None, records.shape[0], seq.ctypes.data if len(seq) else None, seq.shape[0]))


def _as_links(links):
    if not (isinstance(links, np.ndarray) and links.dtype == LINK_DTYPE):
        links = np.array([(int(a), int(b), int(c)) for a, b, c in links], dtype=LINK_DTYPE)
    return np.ascontiguousarray(links)


def links_bubbles(links, n_unitigs, min_link=1, device=0):
    """bgr_links_bubbles: the bubbles of a list of links (an array of LINK_DTYPE, or (from, to, count) triples; canonical, strictly ascending by key,
    as Aligner.links() delivers them) on a graph of n_unitigs unitigs, called on `device` -> array of BUBBLE_DTYPE."""
    links = _as_links(links)
    return _fetch_records(lambda out, cap, n: lib().bgr_links_bubbles(int(device), links.ctypes.data, links.shape[0], int(n_unitigs), int(min_link), out, cap, n), BUBBLE_DTYPE)


def write_bubbles(path, graph, bubbles):
    """bgr_write_bubbles: `bubbles` (an array of BUBBLE_DTYPE) as text -- "#source sink branch1 branch2 len1 len2 in1 out1 in2 out2 kind diff", one
    tab-separated line per bubble."""
    bubbles = np.ascontiguousarray(bubbles, dtype=BUBBLE_DTYPE)
    _check(lib().bgr_write_bubbles(path.encode(), graph.h, bubbles.ctypes.data, bubbles.shape[0]))


def link_canonical(a, b):
    """bgr_link_canonical: the canonical form of the link (a, b) and its 64-bit table key, by the code the kernel runs -> ((from, to), key)."""
    out, key = Link(), C.c_uint64(0)
    _check(lib().bgr_link_canonical(int(a), int(b), C.byref(out), C.byref(key)))
    return (int(out.from_), int(out.to)), int(key.value)


def plan_links(links_bound, n_reads, num_cus=0, form=0):
    """bgr_plan_links: the choice between the links kernel's forms from plain numbers (no device) -> dict as Aligner.links_plan."""
    out = (C.c_uint32 * 4)()
    _check(lib().bgr_plan_links(int(links_bound), int(n_reads), int(num_cus), int(form), out))
    return dict(zip(("form", "blocks", "threads", "lds_bytes"), (int(x) for x in out)))


def write_gfa(path, graph, abundance_rows, links):
    """bgr_write_gfa: GFA 1.0 -- an S line per unitig with RC / KC from `abundance_rows` (n_unitigs, 3), an L line per link of `links` (an array
    of LINK_DTYPE, or (from, to, count) triples), which must be sorted by key as Graph.links() delivers them."""
    rows = np.ascontiguousarray(abundance_rows, dtype=np.uint64)
    if rows.ndim != 2 or rows.shape[1] != 3:
        raise ValueError("write_gfa: abundance_rows must be (n_unitigs, 3)")
    if not (isinstance(links, np.ndarray) and links.dtype == LINK_DTYPE):
        links = np.array([(int(a), int(b), int(c)) for a, b, c in links], dtype=LINK_DTYPE)
    links = np.ascontiguousarray(links)
    _check(lib().bgr_write_gfa(path.encode(), graph.h, rows.ctypes.data, rows.shape[0], links.ctypes.data, links.shape[0]))


def write_abundance(path, graph, rows):
    """bgr_write_abundance: `rows` (n_unitigs, 3) as text -- "#unitig length reads bases kmers", one tab-separated line per unitig."""
    rows = np.ascontiguousarray(rows, dtype=np.uint64)
    if rows.ndim != 2 or rows.shape[1] != 3:
        raise ValueError("write_abundance: rows must be (n_unitigs, 3)")
    _check(lib().bgr_write_abundance(path.encode(), graph.h, rows.ctypes.data, rows.shape[0]))


def load_reads(path, k, fastq=False, threads=1, chunk_bytes=0):
    """getReads (aligner.cpp:46-117) over a whole file -> (reads u8[], read_offs u64[n+1], headers u8[], header_offs u64[n+1])."""
    h = C.c_void_p()
    _check(lib().bgr_readset_load_parallel(path.encode(), int(fastq), k, threads, chunk_bytes, C.byref(h)))
    try:
        n = lib().bgr_readset_count(h)
        r, ro, hd, ho = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_void_p()
        _check(lib().bgr_readset_view(h, C.byref(r), C.byref(ro), C.byref(hd), C.byref(ho)))
        roffs = np.ctypeslib.as_array(C.cast(ro, C.POINTER(C.c_uint64)), shape=(n + 1,)).copy()
        hoffs = np.ctypeslib.as_array(C.cast(ho, C.POINTER(C.c_uint64)), shape=(n + 1,)).copy()
        def _bytes(ptr, total):  # an empty vector hands out a null pointer
            return np.ctypeslib.as_array(C.cast(ptr, C.POINTER(C.c_uint8)), shape=(total,)).copy() if total else np.zeros(0, np.uint8)
        reads = _bytes(r, int(roffs[n]))
        heads = _bytes(hd, int(hoffs[n]))
        return reads, roffs, heads, hoffs
    finally:
        lib().bgr_readset_destroy(h)
