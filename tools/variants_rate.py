#!/usr/bin/env python3
"""SNV sites from an aligner's pileup table: the device path (bgr_aligner_pileup_sites: five launches over the table where it lies, then the
records' copy) against the route there was before it (bgr_aligner_pileup: the table's 20 bytes per base over PCIe and the host conversion, then the
same filter in numpy).  Graphs as tools/pileup_rate.py: bench.py's default Synth shape (genome 4.6 M, spacing 140, 2 alleles) and, with
--only default,chr1, the chr1-scale shape (genome 230 M, spacing 175) if the device holds its table.  k = 31; the table is filled by `--launches`
launches of `--reads` 150 bp reads, m = 2, effort 2.  Then `--reps` repetitions of each path in turn, wall clock end to end; medians, the spread,
the ratio; the five launches' milliseconds of the median-nearest device call (bgr_aligner_pileup_sites_times) and what the classify pass reads per
second: 4 bytes of the difference array per base and word, 16 of the alt words per base with depth >= min_depth.  One JSON line per graph on stdout:
    python tools/variants_rate.py [--launches 4] [--reps 5] [--reads 262144] [--only default] > profiles/variants_rate.txt
The tool does not run bench.py: the `python bench.py` lines of profiles/variants_rate.txt (parent commit and this one, switch off) are appended
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

PRM = (2, 2, 200000)


def numpy_filter(t, ref_codes):
    """the definition over a flat table (array of PILEUP_DTYPE) and the unitigs' letters as codes 0 .. 3 -> the indices of the sites"""
    depth = t["depth"].astype(np.uint64)
    site = np.zeros(len(t), dtype=bool)
    for x, f in enumerate("acgt"):
        c = t[f].astype(np.uint64)
        site |= (ref_codes != x) & (c >= PRM[1]) & (c * np.uint64(1000000) >= np.uint64(PRM[2]) * depth)
    return np.nonzero(site & (depth >= PRM[0]))[0]


def measure(g, seqs, offs, arr, R, L, launches, reps):
    reads = B.DeviceBuffer(0, arr)
    offs_d = B.DeviceBuffer(0, np.arange(R + 1, dtype=np.uint64) * np.uint64(L))
    al = B.Aligner(g, 0)
    al.pileup_enable()
    series(al, reads, offs_d, R, L, launches)
    ref_codes = np.full(256, 4, dtype=np.uint8)
    for i, ch in enumerate(b"ACGT"):
        ref_codes[ch] = i
    ref_codes = ref_codes[np.asarray(seqs, dtype=np.uint8)]
    al.pileup_sites(*PRM)   # (warm: the scratch buffers are allocated)
    dev, host, passes = [], [], []
    n_dev = n_host = None
    for _ in range(reps):   # in turn: what drifts on the machine meets both alike
        t0 = time.perf_counter()
        s = al.pileup_sites(*PRM)
        dev.append(time.perf_counter() - t0)
        passes.append(al.pileup_sites_times())
        n_dev = len(s)
        t0 = time.perf_counter()
        t, _ = al.pileup()
        t1 = time.perf_counter()
        idx = numpy_filter(t, ref_codes)
        host.append((time.perf_counter() - t0, t1 - t0))
        n_host = len(idx)
    covered = int((t["depth"] >= PRM[0]).sum())
    info = g.info()
    T, n = info["total_bases"] // 2, info["n_unitigs"]
    order = sorted(range(reps), key=lambda i: dev[i])
    mid = order[reps // 2]
    hs = sorted(host)
    out = {"sites_device": n_dev, "sites_host_route": n_host, "bases_with_min_depth": covered,
           "device_ms": round(dev[mid] * 1e3, 3), "device_ms_spread": [round(dev[order[0]] * 1e3, 3), round(dev[order[-1]] * 1e3, 3)],
           "host_route_ms": round(hs[reps // 2][0] * 1e3, 1), "host_route_ms_spread": [round(hs[0][0] * 1e3, 1), round(hs[-1][0] * 1e3, 1)],
           "host_route_ms_of_which_bgr_aligner_pileup": round(hs[reps // 2][1] * 1e3, 1),
           "host_over_device": round(hs[reps // 2][0] / dev[mid], 1),
           "passes_ms": dict(zip(("tile_sums", "scan_sums", "classify", "scan_counts", "emit"), (round(x, 4) for x in passes[mid])))}
    classify_bytes = 4 * (T + n) + 16 * covered
    if passes[mid][2] > 0:
        out["classify_bytes"] = classify_bytes
        out["classify_tb_per_s"] = round(classify_bytes / (passes[mid][2] * 1e-3) / 1e12, 3)
        out["classify_share_of_6.29_tb_per_s"] = round(classify_bytes / (passes[mid][2] * 1e-3) / 6.29e12, 3)
    al.close()
    reads.free()
    offs_d.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--reads", type=int, default=262144)
    ap.add_argument("--only", default="default")
    a = ap.parse_args()
    confs = {"default": (4_600_000, 140), "small": (300_000, 140), "chr1": (230_000_000, 175)}
    for name in a.only.split(","):
        R, L = a.reads, 150
        syn = Synth(confs[name][0], confs[name][1], 2, K, 1234)
        seqs, offs = syn.unitigs()
        arr, _ = syn.reads(0, R, L, 2, 4321, threads=16)
        g = B.Graph.build(K, seqs, offs)
        info = g.info()
        r = measure(g, seqs, offs, arr, R, L, a.launches, a.reps)
        r.update(graph=name, n_unitigs=info["n_unitigs"], graph_bases=info["total_bases"] // 2, table_bytes=20 * (info["total_bases"] // 2) + 4 * info["n_unitigs"] + 8,
                 thresholds=list(PRM), reads_per_launch=R, read_len=L, launches=a.launches, reps=a.reps)
        print(json.dumps(r), flush=True)
        g.close()


if __name__ == "__main__":
    main()
