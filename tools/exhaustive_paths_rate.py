#!/usr/bin/env python3
"""Device-resident exhaustive mapping rate (Mreads/s) with the paths of exhaustive launches as output (bgr_aligner_exhaustive_paths_enable): the switch
off, the switch on with nothing counting, and on with abundance, with links + triples and with the pileup -- and the milliseconds of the view kernel
and of each counting kernel from bgr_aligner_kernel_times.  With the switch on and something counting, the counting kernels of a launch are queued
behind its settling (a wait of the host for the launch's cursor block) instead of directly behind the passes: the difference between the series is
what that costs per launch.
Graphs: bench.py's branchy workload (genome 50 M, a site every 36 bp, 4 alleles; 250 bp reads, m = 5) and its default graph (genome 4.6 M, a site every
140 bp, 2 alleles; 150 bp reads, m = 2).  k = 31.  The wall-clock rates are taken without HIP events around the kernels (BGR_KNOB_KERNEL_EVENTS 0, as
bgr_align_all runs): five series of `launches` launches each, the median and the range; the kernel milliseconds in one more series with them.
One JSON line per graph and setting on stdout:
    python tools/exhaustive_paths_rate.py [--launches 10] [--reads 262144] [--only branchy,default] > profiles/exhaustive_paths_rate.txt"""
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
SETTINGS = (("switch off", False, ()), ("switch on", True, ()), ("abundance", True, ("abundance",)), ("links+triples", True, ("links", "triples")), ("pileup", True, ("pileup",)))


def series(al, reads, offs_d, R, L, m, launches):
    """`launches` launches back to back behind a warm-up; the sync at the end settles -- and, with the switch on, counts -- the last one (every other
    launch is settled and counted by the launch behind it)"""
    run = lambda: al.align_device(reads.data_ptr(), offs_d.data_ptr(), R, R * L, L, m=m, effort=2, mode=B.MODE_EXHAUSTIVE)
    run()
    al.sync()
    al.reset_kernel_time()
    t0 = time.perf_counter()
    for _ in range(launches):
        run()
    al.sync()
    return time.perf_counter() - t0


def measure(g, arr, R, L, m, launches, switch, counting):
    out = {}
    reads = B.DeviceBuffer(0, arr)
    offs_d = B.DeviceBuffer(0, np.arange(R + 1, dtype=np.uint64) * np.uint64(L))
    for events in (0, 1):
        al = B.Aligner(g, 0)
        al.set_knob(B.KNOB_KERNEL_EVENTS, events)
        if switch:
            al.exhaustive_paths_enable()
        for what in counting:
            getattr(al, what + "_enable")()
        if events == 0:
            dts = sorted(series(al, reads, offs_d, R, L, m, launches) for _ in range(5))
            out["mreads_per_s"] = round(R * launches / dts[2] / 1e6, 1)   # the median of five series
            out["mreads_per_s_range"] = [round(R * launches / d / 1e6, 1) for d in (dts[4], dts[0])]
            out["ms_per_launch"] = round(dts[2] / launches * 1e3, 4)
        else:
            series(al, reads, offs_d, R, L, m, launches)
            _, slots = al.kernel_times()
            out["kernels_ms_per_launch"] = {n: round(ms / launches, 4) for n, ms in slots}
        al.close()
    reads.free()
    offs_d.free()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--reads", type=int, default=262144)
    ap.add_argument("--only", default="branchy,default")
    a = ap.parse_args()
    confs = {"branchy": (50_000_000, 36, 4, 250, 5), "default": (4_600_000, 140, 2, 150, 2)}
    for name in a.only.split(","):
        genome, spacing, alleles, L, m = confs[name]
        syn = Synth(genome, spacing, alleles, K, 1234)
        seqs, offs = syn.unitigs()
        arr, _ = syn.reads(0, a.reads, L, m, 4321, threads=16)
        g = B.Graph.build(K, seqs, offs)
        base = None
        for label, switch, counting in SETTINGS:
            r = measure(g, arr, a.reads, L, m, a.launches, switch, counting)
            base = r["ms_per_launch"] if base is None else base
            r.update(graph=name, n_unitigs=g.info()["n_unitigs"], setting=label, reads_per_launch=a.reads, read_len=L, max_mismatch=m, launches=a.launches,
                     ms_per_launch_over_switch_off=round(r["ms_per_launch"] - base, 4))
            print(json.dumps(r), flush=True)
        g.close()


if __name__ == "__main__":
    main()
