#!/usr/bin/env python3
"""Device-resident greedy mapping rate (Mreads/s) with the pileup off and on (bgr_aligner_pileup_enable), and the milliseconds of the pileup
kernel next to those of the abundance and links kernels, from bgr_aligner_kernel_times.  Graphs as tools/abundance_rate.py: bench.py's default
Synth shape (genome 4.6 M, spacing 140, 2 alleles), genome 300 k, the chr1-scale shape (genome 230 M, spacing 175), and a skewed one: six
unitigs that every read lands on, where the atomics of a launch meet in a few hundred addresses.  k = 31, 150 bp reads (100 bp on the skewed
graph), m = 2, effort 2.  The wall-clock rates are taken without HIP events around the kernels (BGR_KNOB_KERNEL_EVENTS 0, as bgr_align_all
runs): series of `launches` launches -- off, abundance only, and on -- in turn, the median of `--series` each.  Enabling the pileup enables
unitig abundance, so "on" pays for two kernels behind every launch: the pileup's own share is the step from "abundance" to "on".  The kernel
milliseconds come from a further series with the events, with abundance, links and pileup all counting.  One JSON line per graph on stdout:
    python tools/pileup_rate.py [--launches 10] [--series 5] [--reads 262144] [--only default,small,skewed,chr1] > profiles/pileup_rate.txt
The tool does not run bench.py: the two `python bench.py` lines of profiles/pileup_rate.txt (parent commit and this one, switch off) are
appended to the file by hand."""
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


def measure(g, arr, R, L, launches, n_series):
    out = {}
    reads = B.DeviceBuffer(0, arr)
    offs_d = B.DeviceBuffer(0, np.arange(R + 1, dtype=np.uint64) * np.uint64(L))
    off, ab, on = B.Aligner(g, 0), B.Aligner(g, 0), B.Aligner(g, 0)
    for al in (off, ab, on):
        al.set_knob(B.KNOB_KERNEL_EVENTS, 0)
    ab.abundance_enable()
    on.pileup_enable()   # (and abundance with it)
    dts = {"off": [], "abundance": [], "on": []}
    for _ in range(n_series):   # interleaved: what drifts on the machine meets all alike
        dts["off"].append(series(off, reads, offs_d, R, L, launches))
        dts["abundance"].append(series(ab, reads, offs_d, R, L, launches))
        dts["on"].append(series(on, reads, offs_d, R, L, launches))
    for name in ("off", "abundance", "on"):
        d = sorted(dts[name])
        out["mreads_per_s_" + name] = round(R * launches / d[len(d) // 2] / 1e6, 1)
        out["mreads_per_s_%s_spread" % name] = [round(R * launches / x / 1e6, 1) for x in (d[-1], d[0])]
    n_launches = n_series * (launches + 1)
    out["occurrences_per_launch"] = int(on.abundance()[:, 0].sum()) // n_launches
    if g.info()["total_bases"] < 100_000_000:   # (a delivery moves 20 bytes per base of the graph to the host and converts them there: not for the chr1-scale table here)
        t, skipped = on.pileup()
        out["depth_sum_per_launch"] = int(t["depth"].astype(np.int64).sum()) // n_launches
        out["mismatches_per_launch"] = int(sum(t[f].astype(np.int64).sum() for f in "acgtn")) // n_launches
        out["skipped"] = skipped
    off.close()
    ab.close()
    on.close()
    al = B.Aligner(g, 0)   # the kernels' own times: all three counting kernels behind the mapping passes
    al.set_knob(B.KNOB_KERNEL_EVENTS, 1)
    al.links_enable()
    al.pileup_enable()
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
        info = g.info()
        r = measure(g, arr, R, L, a.launches, a.series)
        r.update(graph=name, n_unitigs=info["n_unitigs"], graph_bases=info["total_bases"] // 2, table_bytes=20 * (info["total_bases"] // 2) + 4 * info["n_unitigs"] + 8,
                 reads_per_launch=R, read_len=L, launches=a.launches, series=a.series)
        print(json.dumps(r), flush=True)
        g.close()


if __name__ == "__main__":
    main()
