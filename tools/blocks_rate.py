#!/usr/bin/env python3
"""What chaining the phased pairs into haplotype blocks costs (bgr_phase_blocks), end to end and per stage, next to the time the definition in
plain Python (tests/blocks_ref.py) needs on the same input -- a yardstick for the reader, not a bar.  The inputs: the bubbles and phase records of
bench.py's default Synth shape (genome 4.6 M, spacing 140, 2 alleles, k = 31; the tables filled by the launches tools/links_rate.py uses) and of the
chr1-scale shape (genome 230 M, spacing 175) when asked for, and crafted lists of --crafted bubbles: one chain through all of them (the deepest
jumping) and chains of 4, ids permuted and signed at random.  --reps repetitions; medians and ranges.  The stages' milliseconds come from HIP events
(bgr_phase_blocks_times: index + link, ranking -- all rounds --, place); `total` is the whole call on the host's clock: two uploads, the
allocation of the scratch, three waits, the entries' way back.  One JSON line per input on stdout:
    python tools/blocks_rate.py [--only default,chain,fours] [--crafted 1000000] [--reps 5] > profiles/blocks_rate.txt"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import bgreat_amd as B  # noqa: E402
import blocks_ref  # noqa: E402
import bubbles_ref  # noqa: E402
import phase_ref  # noqa: E402
from tools.abundance_rate import K, series  # noqa: E402
from tools.bubbles_rate import stats  # noqa: E402
from tools.synth import Synth  # noqa: E402


def crafted(n, run, seed):
    """n bubbles in chains of `run` (n: one chain), every pair decided, cis or trans at random -> (bubbles, phase, n_unitigs) as arrays"""
    rng = np.random.default_rng(seed)
    assert n % run == 0
    chains = n // run
    ids = (rng.permutation(3 * n + chains) + 1).astype(np.int64)
    ids *= rng.choice(np.array([-1, 1]), size=len(ids))
    junction = ids[:n + chains].reshape(chains, run + 1)
    s, t = junction[:, :-1].ravel(), junction[:, 1:].ravel()   # bubble i of the layout: s[i] -> {b[i], c[i]} -> t[i]
    b, c = ids[n + chains:2 * n + chains], ids[2 * n + chains:]
    lo, hi = np.where(np.abs(b) < np.abs(c), b, c), np.where(np.abs(b) < np.abs(c), c, b)
    flip = np.abs(t) < np.abs(s)   # the canonical reading of the record
    bubbles = np.zeros(n, dtype=B.BUBBLE_DTYPE)
    bubbles["source"], bubbles["sink"] = np.where(flip, -t, s), np.where(flip, -s, t)
    bubbles["branch"] = np.stack((np.where(flip, -lo, lo), np.where(flip, -hi, hi)), axis=1)
    bubbles["count"] = 1
    o = lambda x: 2 * (np.abs(x) - 1) + (x < 0)
    bubbles = bubbles[np.argsort(o(bubbles["source"].astype(np.int64)))]
    # the pairs: bubble i and i + 1 of a chain through m = t[i]; in the reading with m > 0 that is X = i, Y = i + 1, else X = mate(i + 1), Y = mate(i)
    x = np.flatnonzero(np.arange(n) % run != run - 1)
    m = t[x]
    fwd = m > 0
    phase = np.zeros(len(x), dtype=B.PHASE_DTYPE)
    phase["via"] = np.abs(m)
    phase["source"], phase["sink"] = np.where(fwd, s[x], -t[x + 1]), np.where(fwd, t[x + 1], -s[x])
    phase["in"] = np.stack((np.where(fwd, lo[x], -lo[x + 1]), np.where(fwd, hi[x], -hi[x + 1])), axis=1)
    phase["out"] = np.stack((np.where(fwd, lo[x + 1], -lo[x]), np.where(fwd, hi[x + 1], -hi[x])), axis=1)
    trans = rng.integers(0, 2, size=len(x)).astype(np.uint64)
    phase["count"] = np.stack((3 - 3 * trans, 3 * trans, 3 * trans, 3 - 3 * trans), axis=1)
    return bubbles, phase[np.argsort(phase["via"])], 3 * n + chains


def of_graph(genome, spacing, reads, launches, note):
    syn = Synth(genome, spacing, 2, K, 1234)
    seqs, offs = syn.unitigs()
    R, L = reads, 150
    arr, _ = syn.reads(0, R, L, 2, 4321, threads=16)
    g = B.Graph.build(K, seqs, offs)
    note("graph built")
    al = B.Aligner(g, 0)
    al.links_enable()
    al.triples_enable()
    rd = B.DeviceBuffer(0, arr)
    od = B.DeviceBuffer(0, np.arange(R + 1, dtype=np.uint64) * np.uint64(L))
    series(al, rd, od, R, L, launches)
    bubbles = al.bubbles(1)
    phase = B.bubbles_phase(bubbles, al.triples())
    n = g.info()["n_unitigs"]
    rd.free()
    od.free()
    al.close()
    g.close()
    return bubbles, phase, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="default,chain,fours")
    ap.add_argument("--crafted", type=int, default=1_000_000)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--reads", type=int, default=262144)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--min-phase", type=int, default=1)
    a = ap.parse_args()
    for name in a.only.split(","):
        t_start = time.perf_counter()
        note = lambda what: print("# %s: %s (%.0f s)" % (name, what, time.perf_counter() - t_start), file=sys.stderr, flush=True)
        if name == "default":
            bubbles, phase, n_unitigs = of_graph(4_600_000, 140, a.reads, a.launches, note)
        elif name == "chr1":
            bubbles, phase, n_unitigs = of_graph(230_000_000, 175, a.reads, a.launches, note)
        else:
            bubbles, phase, n_unitigs = crafted(a.crafted, a.crafted if name == "chain" else 4, 7)
        note("input made")
        B.phase_blocks(bubbles[:64], phase[:0], n_unitigs)   # (the first call of a process loads the kernels)
        total, stages, got = [], {"link": [], "rank": [], "place": []}, None
        for _ in range(a.reps):
            t0 = time.perf_counter()
            got = B.phase_blocks(bubbles, phase, n_unitigs, a.min_phase)
            total.append((time.perf_counter() - t0) * 1e3)
            ms = B.phase_blocks_times()
            for k in stages:
                stages[k].append(ms[k])
        note("device done")
        bt, pt = bubbles_ref.as_tuples(bubbles), phase_ref.as_tuples(phase)
        t0 = time.perf_counter()
        want = blocks_ref.blocks_of(bt, pt, a.min_phase)
        ref_ms = (time.perf_counter() - t0) * 1e3
        assert blocks_ref.as_tuples(got) == want, "the device and the definition disagree"
        sizes = got["size"][got["index"] == 0]
        r = {"input": name, "n_unitigs": int(n_unitigs), "bubbles": int(len(bubbles)), "phase_records": int(len(phase)), "min_phase": a.min_phase, "blocks": int(len(sizes)),
             "blocks_of_more_than_one": int((sizes > 1).sum()), "longest_block": int(sizes.max()) if len(sizes) else 0, "rounds_per_ranking": int(np.ceil(np.log2(max(2, 2 * len(bubbles))))),
             "reps": a.reps, "phase_blocks_ms": stats(total), "link_ms": stats(stages["link"]), "rank_ms": stats(stages["rank"]), "place_ms": stats(stages["place"]),
             "blocks_ref_python_ms": round(ref_ms, 1)}
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
