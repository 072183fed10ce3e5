#!/usr/bin/env python3
"""Device-resident greedy mapping rate (Mreads/s) with unitig abundance off and on (bgr_aligner_abundance_enable), both forms of the abundance
kernel where both apply (BGR_KNOB_ABUNDANCE_FORM), and the kernel's own milliseconds from bgr_aligner_kernel_times.  Graphs: bench.py's default
Synth shape (genome 4.6 M, spacing 140, 2 alleles), a small graph whose table fits a workgroup's LDS (genome 300 k), the chr1-scale shape
(genome 230 M, spacing 175: form A only), and a skewed one: six unitigs that every read lands on.  k = 31, 150 bp reads (100 bp on the skewed
graph), m = 2, effort 2.  The wall-clock rates are taken without HIP events around the kernels (BGR_KNOB_KERNEL_EVENTS 0, as bgr_align_all
runs), the kernel milliseconds in a second series with them.  One JSON line per graph and form on stdout:
    python tools/abundance_rate.py [--launches 10] [--reads 262144] [--only default,small,skewed,chr1] [--e2e-reads 20000000] > profiles/abundance_rate.txt"""
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

K = 31


def skewed(R, L):
    rng = np.random.default_rng(3)
    genome = rng.integers(0, 4, size=390)
    text = np.frombuffer(b"ACGT", dtype=np.uint8)[genome]
    cuts = [0, 65, 130, 195, 260, 325, 390]   # (a cut every 65 bases: every read of 100 spans one, so every read maps)
    parts = [text[max(0, cuts[i] - (K - 1)): cuts[i + 1]] for i in range(len(cuts) - 1)]
    offs = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.uint64)
    starts = rng.integers(0, len(text) - L, size=R)
    reads = text[(starts[:, None] + np.arange(L)[None, :]).ravel()]
    return np.concatenate(parts), offs, np.ascontiguousarray(reads)


def series(al, reads, offs_d, R, L, launches):
    al.align_device(reads.data_ptr(), offs_d.data_ptr(), R, R * L, L, m=2, effort=2)  # warm-up
    al.sync()
    al.reset_kernel_time()
    t0 = time.perf_counter()
    for _ in range(launches):
        al.align_device(reads.data_ptr(), offs_d.data_ptr(), R, R * L, L, m=2, effort=2)
    al.sync()
    return time.perf_counter() - t0


def measure(g, arr, R, L, launches, form):
    """form None = abundance off -> dict(mreads_per_s, kernels_ms_per_launch)"""
    out = {}
    reads = B.DeviceBuffer(0, arr)
    offs_d = B.DeviceBuffer(0, np.arange(R + 1, dtype=np.uint64) * np.uint64(L))
    for events in (0, 1):
        al = B.Aligner(g, 0)
        al.set_knob(B.KNOB_KERNEL_EVENTS, events)
        if form is not None:
            al.set_knob(B.KNOB_ABUNDANCE_FORM, form)
            al.abundance_enable()
        dts = sorted(series(al, reads, offs_d, R, L, launches) for _ in range(3))
        if events == 0:
            out["mreads_per_s"] = round(R * launches / dts[1] / 1e6, 1)   # the median of three series
            out["mreads_per_s_spread"] = [round(R * launches / d / 1e6, 1) for d in (dts[2], dts[0])]
        else:
            _, slots = al.kernel_times()
            out["kernels_ms_per_launch"] = {n: round(ms / launches, 4) for n, ms in slots}
        if form is not None and events == 1:
            out["form"] = "AB"[al.abundance_plan(R, R * L)["form"] - 1]   # the kernel that ran
            t = al.abundance()
            out["occurrences_per_launch"] = int(t[:, 0].sum()) // (3 * (launches + 1))
            out["unitigs_touched"] = int((t[:, 0] > 0).sum())
        al.close()
    reads.free()
    offs_d.free()
    return out


def end_to_end(n, L, threads):
    """bgr_align_all (what the CLI runs) on a FASTA file of n reads written just before, on bench.py's default graph: the whole run with the
    counting off and on, three times each in turn -> one dict"""
    import shutil
    import tempfile
    syn = Synth(4_600_000, 140, 2, K, 20261003)
    g = B.Graph.build(K, *syn.unitigs())
    d = tempfile.mkdtemp(prefix="bgr_abundance_e2e_")
    try:
        f = os.path.join(d, "reads.fa")
        syn.write_reads(f, 0, n, L, 2, 77, threads=threads)
        rates = {False: [], True: []}
        for rep in range(4):   # (the first pair warms the page-locked staging and is dropped)
            for on in (False, True):
                os.sync()
                t0 = time.perf_counter()
                B.align_all(g, f, os.path.join(d, "paths"), os.path.join(d, "notAligned.fa"), m=2, effort=2, threads=threads, abundance=on)
                if rep:
                    rates[on].append(round(n / (time.perf_counter() - t0) / 1e6, 1))
        t = g.abundance()
        return {"graph": "default", "end_to_end": "bgr_align_all, FASTA in, paths + notAligned.fa out", "reads": n, "read_len": L, "file_bytes": os.path.getsize(f),
                "host_threads": threads, "mreads_per_s_off": rates[False], "mreads_per_s_on": rates[True], "occurrences": int(t[:, 0].sum()), "n_unitigs": g.info()["n_unitigs"]}
    finally:
        shutil.rmtree(d)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--reads", type=int, default=262144)
    ap.add_argument("--only", default="default,small,skewed,chr1")
    ap.add_argument("--e2e-reads", type=int, default=0, help="also one end-to-end leg: a FASTA file of this many 150 bp reads through bgr_align_all, off and on")
    ap.add_argument("--threads", type=int, default=16)
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
        for label, form in (("off", None), ("A", B.ABUNDANCE_GLOBAL), ("B", B.ABUNDANCE_LDS), ("auto", B.ABUNDANCE_AUTO)):
            if label == "B" and 12 * (n_unitigs + 1) > 160 * 1024:
                continue   # (no workgroup holds the table: the knob would run form A)
            r = measure(g, arr, R, L, a.launches, form)
            r.update(graph=name, n_unitigs=n_unitigs, abundance=label, reads_per_launch=R, read_len=L, launches=a.launches)
            print(json.dumps(r), flush=True)
        g.close()
    if a.e2e_reads:
        print(json.dumps(end_to_end(a.e2e_reads, 150, a.threads)), flush=True)


if __name__ == "__main__":
    main()
