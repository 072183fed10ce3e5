#!/usr/bin/env python3
"""How many anchor-scan steps does bgr_align_greedy_multi_kernel take?  Per-wave counts of the last launch (scan steps, items scanned, groups
of items a wave took), summed over the launch: the measured counterpart of tools/scan_halves.py's model, every item included (follow-up
items and reverse complements too).  Counted by the two-scanner scan of the table-in-LDS instances only.
Needs the diagnostic build (make -C bgreat_amd BUILD=build_phase LIBDIR=lib_phase EXTRA=-DBGR_PHASE_TIMING lib_phase/libbgreat_gpu.so) loaded
through BGR_LIB_PATH.  usage (GPU box): BGR_LIB_PATH=... python tools/scan_steps.py [--workload ecoli|small] [--reads N]"""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bgreat_amd as B  # noqa: E402
from tools.synth import Synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--workload", default="ecoli", choices=["ecoli", "small"])
ap.add_argument("--reads", type=int, default=0)
args = ap.parse_args()
G, d, L, R = {"ecoli": (4_600_000, 140, 150, 5_000_000), "small": (250_000, 75, 100, 1_000_000)}[args.workload]
R = args.reads or R
s = Synth(G, d, 2, 31, 20261003)
seqs, offs = s.unitigs()
g = B.Graph.build(31, seqs, offs)
al = B.Aligner(g, 0)
reads, _ = s.reads(0, R, L, 2, 77, threads=16)
db = B.DeviceBuffer(0, reads)
do = B.DeviceBuffer(0, np.arange(R + 1, dtype=np.uint64) * np.uint64(L))
al.align_device(db.data_ptr(), do.data_ptr(), R, R * L, L, m=2, effort=2, mode=0)
al.sync()
lib = B.lib()
lib.bgr_debug_scan_counts.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
n = C.c_uint64()
B._check(lib.bgr_debug_scan_counts(al.h, None, 0, C.byref(n)))
buf = np.zeros(4 * n.value, dtype=np.uint64)
B._check(lib.bgr_debug_scan_counts(al.h, buf.ctypes.data, n.value, C.byref(n)))
w = buf.reshape(-1, 4)
lo32, sh32 = np.uint64(0xFFFFFFFF), np.uint64(32)
steps, items, groups = float(w[:, 0].sum()), float((w[:, 1] & lo32).sum()), float((w[:, 2] & lo32).sum())
# the jump in front of the scan (graphs with a jump index): items it settled without a scan step (not among the items scanned), items whose
# resume position it raised (tools/scan_jump.py is the model)
jumped, raised = float((w[:, 3] & lo32).sum()), float((w[:, 3] >> sh32).sum())
# of the settled ones: by the far entry; of the scanned ones: those left a range the jump cut at either end (raised ones are among them)
by_far, bounded = float((w[:, 1] >> sh32).sum()), float((w[:, 2] >> sh32).sum())
print("workload %s, %d reads, %d waves (launch %s)" % (args.workload, R, n.value, al.launch_info()))
print("scan steps %d, items scanned %d (%.3f per read), groups of items %d (%.2f items each)" % (steps, items, items / R, groups, items / max(groups, 1)))
print("jump index: %s; items settled by the jump %d (%.1f %% of all items), resume position raised %d (%.1f %%)" % (
    g.jump_info()["jump_entries"] or "none", jumped, 100 * jumped / max(items + jumped, 1), raised, 100 * raised / max(items + jumped, 1)))
print("            settled by the far entry %d (%.1f %%), scanned a bounded range %d (%.1f %%)" % (
    by_far, 100 * by_far / max(items + jumped, 1), bounded, 100 * bounded / max(items + jumped, 1)))
print("steps per sixteen items, settled ones included: %.2f" % (16 * steps / max(items + jumped, 1)))
print("steps per read %.3f, per item %.3f, per sixteen items %.2f, per group %.2f" % (steps / R, steps / max(items, 1), 16 * steps / max(items, 1), steps / max(groups, 1)))
