#!/usr/bin/env python3
"""Device-resident greedy mapping rate (Mreads/s) with counting off, with the pileup on (bgr_aligner_pileup_enable) and with the pileup and its
strands on (bgr_aligner_pileup_strands_enable), and the milliseconds of the pileup kernel in both forms, from bgr_aligner_kernel_times.  Graphs,
reads and launches are those of tools/pileup_rate.py: bench.py's default Synth shape, genome 300 k, the chr1-scale shape, and the skewed one (six
unitigs that every read lands on: the pileup's known contention limit, where the second table's atomics meet in the same few hundred addresses
again).  The wall-clock rates are taken without HIP events around the kernels: series of `launches` launches -- off, pileup, pileup + strands -- in
turn, the median of `--series` each.  The kernel milliseconds come from two further series with the events, one aligner per form.  On the default
graph the site calls follow: bgr_aligner_pileup_strand_sites next to bgr_aligner_pileup_sites on the same aligner's tables (the sum of the five
launches, the median of `--series` calls each, in turn).  One JSON line per graph on stdout:
    python tools/strands_rate.py [--launches 10] [--series 5] [--reads 262144] [--only default,small,skewed,chr1] > profiles/strands_rate.txt
The tool does not run bench.py or tools/pileup_rate.py: their lines in profiles/strands_rate.txt (parent commit and this one, switches off) are
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

FORMS = ("off", "pileup", "strands")


def measure(g, arr, R, L, launches, n_series, sites):
    out = {}
    reads = B.DeviceBuffer(0, arr)
    offs_d = B.DeviceBuffer(0, np.arange(R + 1, dtype=np.uint64) * np.uint64(L))
    als = {name: B.Aligner(g, 0) for name in FORMS}
    for al in als.values():
        al.set_knob(B.KNOB_KERNEL_EVENTS, 0)
    als["pileup"].pileup_enable()
    als["strands"].pileup_strands_enable()   # (and the pileup, and abundance, with it)
    dts = {name: [] for name in FORMS}
    for _ in range(n_series):   # interleaved: what drifts on the machine meets all alike
        for name in FORMS:
            dts[name].append(series(als[name], reads, offs_d, R, L, launches))
    for name in FORMS:
        d = sorted(dts[name])
        out["mreads_per_s_" + name] = round(R * launches / d[len(d) // 2] / 1e6, 1)
        out["mreads_per_s_%s_spread" % name] = [round(R * launches / x / 1e6, 1) for x in (d[-1], d[0])]
    n_launches = n_series * (launches + 1)
    if g.info()["total_bases"] < 100_000_000:   # (a delivery moves 20 bytes per base to the host and converts them there: not for the chr1-scale tables)
        t, skipped = als["strands"].pileup()
        f = als["strands"].pileup_forward()
        out["depth_sum_per_launch"] = int(t["depth"].astype(np.int64).sum()) // n_launches
        out["forward_depth_sum_per_launch"] = int(f["depth"].astype(np.int64).sum()) // n_launches
        out["mismatches_per_launch"] = int(sum(t[c].astype(np.int64).sum() for c in "acgtn")) // n_launches
        out["forward_mismatches_per_launch"] = int(sum(f[c].astype(np.int64).sum() for c in "acgtn")) // n_launches
        assert all((f[c] <= t[c]).all() for c in ("depth",) + tuple("acgtn"))
    if sites:   # on the tables these launches filled
        al = als["strands"]
        al.set_knob(B.KNOB_KERNEL_EVENTS, 1)
        ms = {"sites": [], "strand_sites": []}
        for _ in range(n_series):
            n_plain = len(al.pileup_sites(2, 2, 200000))
            ms["sites"].append(sum(al.pileup_sites_times()))
            n_strand = len(al.pileup_strand_sites(2, 2, 200000, 1))
            ms["strand_sites"].append(sum(al.pileup_sites_times()))
        out["sites_ms"] = round(sorted(ms["sites"])[n_series // 2], 4)
        out["strand_sites_ms"] = round(sorted(ms["strand_sites"])[n_series // 2], 4)
        out["n_sites"], out["n_strand_sites_min_alt_strand_1"] = n_plain, n_strand
    for al in als.values():
        al.close()
    out["kernels_ms_per_launch"] = {}
    for name in ("pileup", "strands"):   # the kernels' own times, one aligner per form
        al = B.Aligner(g, 0)
        al.set_knob(B.KNOB_KERNEL_EVENTS, 1)
        (al.pileup_enable if name == "pileup" else al.pileup_strands_enable)()
        series(al, reads, offs_d, R, L, launches)
        _, slots = al.kernel_times()
        out["kernels_ms_per_launch"][name] = {n: round(ms / launches, 4) for n, ms in slots}
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
        r = measure(g, arr, R, L, a.launches, a.series, sites=name == "default")
        r.update(graph=name, n_unitigs=info["n_unitigs"], graph_bases=info["total_bases"] // 2, table_bytes=2 * (20 * (info["total_bases"] // 2) + 4 * info["n_unitigs"] + 8),
                 reads_per_launch=R, read_len=L, launches=a.launches, series=a.series)
        print(json.dumps(r), flush=True)
        g.close()


if __name__ == "__main__":
    main()
