#!/usr/bin/env python3
"""Device-resident greedy mapping rate (Mreads/s) of two-word overlap keys next to the one-word path, on bench.py's E. coli-scale Synth
shape (genome 4.6 M, spacing 140, 2 alleles), 5 M x 150 bp reads per launch, m = 2, effort 2.  Four configurations: k = 31 (default
launch), k = 31 with the general kernel only (BGR_KNOB_GREEDY_FAST), k = 31 built under test.wide_keys (bgr_align_greedy_wide_kernel),
k = 63.  One JSON line per configuration on stdout:  python tools/wide_rate.py [--launches 5] > profiles/wide_rate.txt"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import bgreat_amd as B  # noqa: E402
from tools.synth import Synth  # noqa: E402


def rate(k, wide_keys, general_only, launches, R, L):
    syn = Synth(4_600_000, 140, 2, k, 1234)
    seqs, offs = syn.unitigs()
    with B.options(**{"test.wide_keys": wide_keys}):
        g = B.Graph.build(k, seqs, offs)
    al = B.Aligner(g, 0)
    if general_only:
        al.set_knob(B.KNOB_GREEDY_FAST, 1)
    arr, _ = syn.reads(0, R, L, 2, 4321, threads=16)
    reads = B.DeviceBuffer(0, arr)
    offs_d = B.DeviceBuffer(0, np.arange(R + 1, dtype=np.uint64) * np.uint64(L))
    al.align_device(reads.data_ptr(), offs_d.data_ptr(), R, R * L, L, m=2, effort=2)  # warm-up
    al.sync()
    al.reset_kernel_time()
    al.reset_counters()
    t0 = time.perf_counter()
    for _ in range(launches):
        al.align_device(reads.data_ptr(), offs_d.data_ptr(), R, R * L, L, m=2, effort=2)
    al.sync()
    dt = time.perf_counter() - t0
    _, slots = al.kernel_times()
    c = al.counters()
    out = dict(k=k, wide_keys=wide_keys, general_kernel_only=general_only, reads_per_launch=R, launches=launches, mreads_per_s=round(R * launches / dt / 1e6, 1),
               kernels_ms_per_launch={n: round(ms / launches, 3) for n, ms in slots}, aligned_share=round(c["aligned"] / max(1, c["reads"]), 4),
               info=al.launch_info())
    reads.free()
    offs_d.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--reads", type=int, default=5_000_000)
    ap.add_argument("--only", default="", help="comma list of configurations to run (k31,k31_general,k31_wide,k63)")
    a = ap.parse_args()
    confs = {"k31": (31, 0, False), "k31_general": (31, 0, True), "k31_wide": (31, 1, False), "k63": (63, 0, False)}
    for name, (k, w, gen) in confs.items():
        if a.only and name not in a.only.split(","):
            continue
        r = rate(k, w, gen, a.launches, a.reads, 150)
        r["config"] = name
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
