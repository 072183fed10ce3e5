#!/usr/bin/env python3
"""What calling the bubbles costs (bgr_aligner_bubbles) against the route a library caller had before it: the aligner's table of links to the
host (bgr_aligner_links: the whole table crosses, is compacted and sorted there) and the same rule in numpy.  The graphs are bench.py's
default Synth shape (genome 4.6 M, spacing 140, 2 alleles) and the chr1-scale shape (genome 230 M, spacing 175), k = 31, the tables filled by
the launches tools/links_rate.py uses (262 144 reads of 150 bp per launch, m = 2, effort 2).  Five repetitions of each route, in turn;
medians and ranges.  The four launches' milliseconds come from HIP events (bgr_aligner_bubbles_times: adjacency -- with the memset of the
degrees in front of it --, count, scan, emit).  One JSON line per graph on stdout:
    python tools/bubbles_rate.py [--launches 10] [--reads 262144] [--only default,chr1] [--reps 5] > profiles/bubbles_rate.txt"""
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


def bubbles_numpy(links, n, min_link=1):
    """the definition (include/bgreat_gpu.h, bgr_bubble) over an array of LINK_DTYPE -> array of BUBBLE_DTYPE, vectorised"""
    l = links[links["count"] >= min_link]
    a, b, c = l["from"].astype(np.int64), l["to"].astype(np.int64), l["count"]
    m = b != -a   # (a link that is its own strand mate is one edge)
    frm, to, cnt = np.concatenate((a, -b[m])), np.concatenate((b, -a[m])), np.concatenate((c, c[m]))
    o = lambda x: 2 * (np.abs(x) - 1) + (x < 0)
    of = o(frm)
    deg = np.bincount(of, minlength=2 * n)
    order = np.argsort(of, kind="stable")
    to, cnt = to[order], cnt[order]
    first = np.searchsorted(of[order], np.arange(2 * n))   # where the successors of an oriented id start
    s = np.flatnonzero(deg == 2)
    sb, sc = first[s], first[s] + 1
    swap = o(to[sc]) < o(to[sb])   # the branches in (|id|, id < 0) order
    sb, sc = np.where(swap, sc, sb), np.where(swap, sb, sc)
    bb, cc = to[sb], to[sc]
    ob, oc = o(bb), o(cc)
    ok = (deg[ob ^ 1] == 1) & (deg[oc ^ 1] == 1) & (deg[ob] == 1) & (deg[oc] == 1)
    s, sb, sc, bb, cc, ob, oc = (x[ok] for x in (s, sb, sc, bb, cc, ob, oc))
    t = to[first[ob]]
    ok = (t == to[first[oc]]) & (deg[o(t) ^ 1] == 2)
    sid = np.where(s & 1, -(s >> 1) - 1, (s >> 1) + 1)
    ids = np.stack((np.abs(sid), np.abs(bb), np.abs(cc), np.abs(t)))
    for i in range(4):
        for j in range(i + 1, 4):
            ok &= ids[i] != ids[j]
    ok &= np.abs(sid) < np.abs(t)   # of the two strands the one with the smaller (s, t)
    out = np.zeros(int(ok.sum()), dtype=B.BUBBLE_DTYPE)
    out["source"], out["sink"] = sid[ok], t[ok]
    out["branch"] = np.stack((bb[ok], cc[ok]), axis=1)
    out["count"] = np.stack((cnt[sb[ok]], cnt[first[ob[ok]]], cnt[sc[ok]], cnt[first[oc[ok]]]), axis=1)
    return out


def stats(xs):
    xs = sorted(xs)
    return {"median": round(xs[len(xs) // 2], 3), "range": [round(xs[0], 3), round(xs[-1], 3)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--reads", type=int, default=262144)
    ap.add_argument("--only", default="default,chr1")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--min-link", type=int, default=1)
    a = ap.parse_args()
    confs = {"default": (4_600_000, 140), "chr1": (230_000_000, 175)}
    R, L = a.reads, 150
    for name in a.only.split(","):
        note = lambda what: print("# %s: %s (%.0f s)" % (name, what, time.perf_counter() - t_start), file=sys.stderr, flush=True)
        t_start = time.perf_counter()
        syn = Synth(confs[name][0], confs[name][1], 2, K, 1234)
        seqs, offs = syn.unitigs()
        arr, _ = syn.reads(0, R, L, 2, 4321, threads=16)
        note("unitigs and reads made")
        g = B.Graph.build(K, seqs, offs)
        note("graph built")
        n = g.info()["n_unitigs"]
        al = B.Aligner(g, 0)
        al.links_enable()
        reads = B.DeviceBuffer(0, arr)
        offs_d = B.DeviceBuffer(0, np.arange(R + 1, dtype=np.uint64) * np.uint64(L))
        series(al, reads, offs_d, R, L, a.launches)
        info = al.links_info()
        note("table filled")
        dev, host_links, host_rule, passes = [], [], [], [[], [], [], []]
        got = want = None
        for _ in range(a.reps):   # in turn
            t0 = time.perf_counter()
            got = al.bubbles(a.min_link)
            dev.append((time.perf_counter() - t0) * 1e3)
            for i, ms in enumerate(al.bubbles_times()):
                passes[i].append(ms)
            t0 = time.perf_counter()
            links = al.links()
            t1 = time.perf_counter()
            want = bubbles_numpy(links, n, a.min_link)
            host_links.append((t1 - t0) * 1e3)
            host_rule.append((time.perf_counter() - t1) * 1e3)
        assert got.tobytes() == want.tobytes(), "the two routes disagree"
        table_bytes = 16 * info["capacity"]
        r = {"graph": name, "n_unitigs": n, "table_slots": info["capacity"], "table_bytes": table_bytes, "links": int(len(links)), "min_link": a.min_link, "bubbles": int(len(got)),
             "reads_per_launch": R, "launches": a.launches + 1, "reps": a.reps,
             "aligner_bubbles_ms": stats(dev), "adjacency_ms": stats(passes[0]), "count_ms": stats(passes[1]), "scan_ms": stats(passes[2]), "emit_ms": stats(passes[3]),
             "adjacency_read_GBps": round(table_bytes / (stats(passes[0])["median"] * 1e-3) / 1e9, 1),
             "host_route_ms": stats([x + y for x, y in zip(host_links, host_rule)]), "host_links_ms": stats(host_links), "host_numpy_rule_ms": stats(host_rule),
             "scratch_bytes": 56 * n}
        print(json.dumps(r), flush=True)
        reads.free()
        offs_d.free()
        al.close()
        g.close()


if __name__ == "__main__":
    main()
