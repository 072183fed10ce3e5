#!/usr/bin/env python3
"""Device-resident greedy mapping rate (Mreads/s) with counting off, with link counting on (bgr_aligner_links_enable, the automatic form) and
with links + triples on (bgr_aligner_triples_enable), and the kernels' own milliseconds from bgr_aligner_kernel_times.  The graphs and the
launches are those of tools/links_rate.py, so that a line here stands next to the links kernel's line for the same graph in
profiles/links_rate.txt: bench.py's default Synth shape (genome 4.6 M, spacing 140, 2 alleles), a small graph (genome 300 k), the chr1-scale
shape (genome 230 M, spacing 175), and a skewed one: six unitigs that every read lands on.  k = 31, 150 bp reads (100 bp on the skewed graph),
m = 2, effort 2.  The wall-clock rates are taken without HIP events around the kernels (BGR_KNOB_KERNEL_EVENTS 0, as bgr_align_all runs), the
kernel milliseconds in a second series with them.  Every line also has the graph's bound of distinct triples and the bytes of the table an
aligner allocates for it.  One JSON line per graph and setting on stdout:
    python tools/triples_rate.py [--launches 10] [--reads 262144] [--only default,small,skewed,chr1] > profiles/triples_rate.txt"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import bgreat_amd as B  # noqa: E402
from tools.abundance_rate import K, series, skewed  # noqa: E402
from tools.synth import Synth  # noqa: E402


def measure(g, arr, R, L, launches, links, triples):
    """-> dict(mreads_per_s, kernels_ms_per_launch, ...)"""
    out = {}
    reads = B.DeviceBuffer(0, arr)
    offs_d = B.DeviceBuffer(0, np.arange(R + 1, dtype=np.uint64) * np.uint64(L))
    for events in (0, 1):
        al = B.Aligner(g, 0)
        al.set_knob(B.KNOB_KERNEL_EVENTS, events)
        if links:
            al.links_enable()
        if triples:
            al.triples_enable()
        dts = sorted(series(al, reads, offs_d, R, L, launches) for _ in range(3))
        if events == 0:
            out["mreads_per_s"] = round(R * launches / dts[1] / 1e6, 1)   # the median of three series
            out["mreads_per_s_spread"] = [round(R * launches / d / 1e6, 1) for d in (dts[2], dts[0])]
        else:
            _, slots = al.kernel_times()
            out["kernels_ms_per_launch"] = {n: round(ms / launches, 4) for n, ms in slots}
        if triples and events == 1:
            info = al.triples_info()
            t = al.triples()
            out["traversals_per_launch"] = int(t["count"].sum()) // (3 * (launches + 1))
            out["triples_touched"] = len(t)
            out["table_slots"] = info["capacity"]
            out["table_bytes"] = 24 * info["capacity"] + 16
            out["overflow"] = info["overflow"]
        al.close()
    reads.free()
    offs_d.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--reads", type=int, default=262144)
    ap.add_argument("--only", default="default,small,skewed,chr1")
    a = ap.parse_args()
    confs = {"default": (4_600_000, 140), "small": (300_000, 140), "chr1": (230_000_000, 175), "skewed": None}
    for name in a.only.split(","):
        R = a.reads
        if confs[name] is None:
            L = 100
            seqs, offs, arr = skewed(R, L)
        else:
            L = 150
            syn = Synth(confs[name][0], confs[name][1], 2, K, 1234)
            seqs, offs = syn.unitigs()
            arr, _ = syn.reads(0, R, L, 2, 4321, threads=16)
        g = B.Graph.build(K, seqs, offs)
        n_unitigs = g.info()["n_unitigs"]
        bounds = dict(links_bound=g.links_bound(), triples_bound=g.triples_bound())
        for label, links, triples in (("off", False, False), ("links", True, False), ("links+triples", True, True)):
            r = measure(g, arr, R, L, a.launches, links, triples)
            r.update(graph=name, n_unitigs=n_unitigs, counting=label, reads_per_launch=R, read_len=L, launches=a.launches, **bounds)
            print(json.dumps(r), flush=True)
        g.close()


if __name__ == "__main__":
    main()
