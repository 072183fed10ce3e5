#!/usr/bin/env python3
"""Device-resident greedy mapping rate (Mreads/s) with the inside pass off and on (bgr_aligner_inside_enable), the milliseconds of
bgr_align_inside_kernel next to those of the mapping passes (bgr_aligner_kernel_times), the share of the reads without an anchor and the share
of those the pass maps, the index's bytes and build time, and the rate of anchors mode (-G) on the same reads: what a user had before.
Graphs as tools/pileup_rate.py: bench.py's default Synth shape (genome 4.6 M, spacing 140, 2 alleles), genome 300 k, the chr1-scale shape
(genome 230 M, spacing 175).  k = 31, 150 bp reads, m = 2, effort 2.  The wall-clock rates are taken without HIP events around the kernels
(BGR_KNOB_KERNEL_EVENTS 0, as bgr_align_all runs): series of `launches` launches -- off, on, anchors -- in turn, the median of `--series`
each with the slowest and the fastest.  The kernel milliseconds come from a further series with the events.  One JSON line per graph:
    python tools/inside_rate.py [--launches 10] [--series 5] [--reads 262144] [--only default,small,chr1] [--no-anchors] > profiles/inside_rate.txt
The tool does not run bench.py: the `python bench.py` lines of profiles/inside_rate.txt (parent commit and this one, switch off) are appended
to the file by hand."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

import bgreat_amd as B  # noqa: E402
from tools.abundance_rate import K, series  # noqa: E402
from tools.synth import Synth  # noqa: E402


def series_mode(al, reads, offs_d, R, L, launches, mode):
    al.align_device(reads.data_ptr(), offs_d.data_ptr(), R, R * L, L, m=2, effort=2, mode=mode)  # warm-up
    al.sync()
    t0 = time.perf_counter()
    for _ in range(launches):
        al.align_device(reads.data_ptr(), offs_d.data_ptr(), R, R * L, L, m=2, effort=2, mode=mode)
    al.sync()
    return time.perf_counter() - t0


def rates(out, name, dts, R, launches):
    d = sorted(dts)
    out["mreads_per_s_" + name] = round(R * launches / d[len(d) // 2] / 1e6, 1)
    out["mreads_per_s_%s_spread" % name] = [round(R * launches / x / 1e6, 1) for x in (d[-1], d[0])]


def measure(g, ga, arr, R, L, launches, n_series):
    out = {}
    reads = B.DeviceBuffer(0, arr)
    offs_d = B.DeviceBuffer(0, np.arange(R + 1, dtype=np.uint64) * np.uint64(L))
    off, on = B.Aligner(g, 0), B.Aligner(g, 0)
    anc = B.Aligner(ga, 0) if ga is not None else None
    for al in (off, on, anc):
        if al is not None:
            al.set_knob(B.KNOB_KERNEL_EVENTS, 0)
    on.inside_enable()
    dts = {"off": [], "on": [], "anchors": []}
    for _ in range(n_series):   # interleaved: what drifts on the machine meets all alike
        dts["off"].append(series(off, reads, offs_d, R, L, launches))
        dts["on"].append(series(on, reads, offs_d, R, L, launches))
        if anc is not None:
            dts["anchors"].append(series_mode(anc, reads, offs_d, R, L, launches, B.MODE_ANCHORS))
    rates(out, "off", dts["off"], R, launches)
    rates(out, "on", dts["on"], R, launches)
    if anc is not None:
        rates(out, "anchors_mode", dts["anchors"], R, launches)
    n_launches = n_series * (launches + 1)
    c = off.counters()
    out["share_no_anchor"] = round(c["no_overlap"] / max(1, c["reads"]), 4)
    out["share_of_those_mapped_inside"] = round(on.inside_count() / n_launches / max(1, c["no_overlap"] / n_launches), 4)
    for al in (off, on, anc):
        if al is not None:
            al.close()
    al = B.Aligner(g, 0)   # the kernels' own times
    al.set_knob(B.KNOB_KERNEL_EVENTS, 1)
    al.inside_enable()
    series(al, reads, offs_d, R, L, launches)
    _, slots = al.kernel_times()
    out["kernels_ms_per_launch"] = {n: round(ms / launches, 4) for n, ms in slots}
    al.close()
    reads.free()
    offs_d.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--series", type=int, default=5)
    ap.add_argument("--reads", type=int, default=262144)
    ap.add_argument("--only", default="default,small,chr1")
    ap.add_argument("--no-anchors", action="store_true", help="leave out the -G series (its index costs ~9.5 bytes per graph base and minutes at chr1 scale)")
    a = ap.parse_args()
    confs = {"default": (4_600_000, 140), "small": (300_000, 140), "chr1": (230_000_000, 175)}
    for name in a.only.split(","):
        R, L = a.reads, 150
        syn = Synth(confs[name][0], confs[name][1], 2, K, 1234)
        seqs, offs = syn.unitigs()
        arr, _ = syn.reads(0, R, L, 2, 4321, threads=16)
        g = B.Graph.build(K, seqs, offs)
        g.inside_build()
        ga = None if a.no_anchors else B.Graph.build(K, seqs, offs, anchors=True)
        info, ii = g.info(), g.inside_info()
        r = measure(g, ga, arr, R, L, a.launches, a.series)
        r.update(graph=name, n_unitigs=info["n_unitigs"], graph_bases=info["total_bases"] // 2, index_entries=ii["entries"], index_slots=ii["slots"], index_bytes=ii["bytes"],
                 index_bytes_per_graph_base=round(ii["bytes"] / (info["total_bases"] // 2), 2), index_build_seconds=round(ii["build_seconds"], 3),
                 reads_per_launch=R, read_len=L, launches=a.launches, series=a.series)
        print(json.dumps(r), flush=True)
        g.close()
        if ga is not None:
            ga.close()


if __name__ == "__main__":
    main()
