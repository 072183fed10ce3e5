#!/usr/bin/env python3
"""What spelling the haplotypes' sequences costs (bgr_blocks_haplotypes), end to end and per stage, with the spell pass in GB/s of written bytes next
to the device's streaming-copy figure, and next to the time the host needs for the same bytes with a plain numpy gather over the unitigs' characters
(the walks from tests/haplotypes_ref.py) -- a yardstick for the reader, not a bar.  The inputs: bench.py's default Synth shape (genome 4.6 M, spacing
140, 2 alleles, k = 31) with the bubbles, phase records and blocks of the eleven launches tools/blocks_rate.py uses, and a crafted case: --crafted
bubbles in chains of four over random unitigs of --unitig-len characters (tools/blocks_rate.py's lists; every junction is bad there, and counted),
which gives a few hundred MB of output.  --reps repetitions; medians and ranges.  The stages' milliseconds come from HIP events
(bgr_blocks_haplotypes_times: items + scan, spell -- from an event recorded behind the allocation of the output to one behind the kernel --, records);
`blocks_haplotypes_ms` is the whole C call that delivers the bytes, on the host's clock inside the library: two uploads, the allocations, three waits,
the records' and the characters' way back.  `python_wrapper_ms` is bgreat_amd.blocks_haplotypes around it, which makes a sizing call first (both
uploads and the first two passes once more) and allocates the two numpy arrays.  One JSON line per input on stdout:
    python tools/haplotypes_rate.py [--only default,crafted] [--crafted 24000] [--unitig-len 3000] [--reps 5] > profiles/haplotypes_rate.txt"""
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
import haplotypes_ref  # noqa: E402
from tools.abundance_rate import K, series  # noqa: E402
from tools.blocks_rate import crafted  # noqa: E402
from tools.bubbles_rate import stats  # noqa: E402
from tools.synth import Synth  # noqa: E402

STREAM_COPY_TBS = 6.29   # the streaming-copy figure the README quotes for one MI355X


def of_graph(genome, spacing, reads, launches, note):
    """-> (graph resident on device 0, unitig characters, offsets, bubbles, entries)"""
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
    entries = B.phase_blocks(bubbles, phase, g.info()["n_unitigs"])
    rd.free()
    od.free()
    al.close()
    g.upload(0)
    return g, seqs, offs, bubbles, entries


def of_crafted(n, unitig_len, note):
    bubbles, phase, n_unitigs = crafted(n, 4, 7)
    rng = np.random.default_rng(11)
    seqs = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n_unitigs * unitig_len)]
    offs = np.arange(n_unitigs + 1, dtype=np.uint64) * np.uint64(unitig_len)
    g = B.Graph.build(K, seqs, offs)
    note("graph built")
    g.upload(0)
    return g, seqs, offs, bubbles, B.phase_blocks(bubbles, phase, n_unitigs)


def host_spell(seqs, offs, k, bubbles, entries):
    """the same bytes on the host: the walks in Python, the characters by numpy slices of the forward text and of its reverse complement"""
    comp = np.zeros(256, dtype=np.uint8)
    comp[np.frombuffer(b"ACGT", dtype=np.uint8)] = np.frombuffer(b"TGCA", dtype=np.uint8)
    back = comp[seqs][::-1]   # the reverse complement of the whole text: unitig i lies at [total - offs[i + 1], total - offs[i])
    total = int(offs[-1])
    parts = []
    for block in haplotypes_ref.blocks_in(entries):
        for walk in haplotypes_ref.walks_of(block, bubbles):
            for j, x in enumerate(walk):
                a, b = int(offs[abs(x) - 1]), int(offs[abs(x)])
                piece = seqs[a:b] if x > 0 else back[total - b:total - a]
                parts.append(piece[k - 1:] if j else piece)
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="default,crafted")
    ap.add_argument("--crafted", type=int, default=24000)
    ap.add_argument("--unitig-len", type=int, default=3000)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--reads", type=int, default=262144)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--min-block", type=int, default=1)
    a = ap.parse_args()
    for name in a.only.split(","):
        t_start = time.perf_counter()
        note = lambda what: print("# %s: %s (%.0f s)" % (name, what, time.perf_counter() - t_start), file=sys.stderr, flush=True)
        if name == "default":
            g, seqs, offs, bubbles, entries = of_graph(4_600_000, 140, a.reads, a.launches, note)
        else:
            g, seqs, offs, bubbles, entries = of_crafted(a.crafted, a.unitig_len, note)
        note("input made")
        B.blocks_haplotypes(g, bubbles, entries[:0])
        B.blocks_haplotypes(g, bubbles[:1], np.array([(1, 0, 1, 0, 0, 0)], dtype=B.BLOCK_DTYPE))   # (the first call of a process loads the kernels)
        total, wrapper, stages, got = [], [], {"items": [], "spell": [], "records": []}, None
        for _ in range(a.reps):
            t0 = time.perf_counter()
            got = B.blocks_haplotypes(g, bubbles, entries, a.min_block)
            wrapper.append((time.perf_counter() - t0) * 1e3)
            ms = B.blocks_haplotypes_times()   # (of the wrapper's second call, the one that delivers)
            total.append(ms["total"])
            for key in stages:
                stages[key].append(ms[key])
        note("device done")
        recs, data, bad = got
        bt, et = bubbles_ref.as_tuples(bubbles), blocks_ref.as_tuples(entries)
        t0 = time.perf_counter()
        want = host_spell(seqs, offs, K, bt, et) if a.min_block == 1 else None
        host_ms = (time.perf_counter() - t0) * 1e3
        if want is not None:
            assert np.array_equal(want, data), "the device and the host gather disagree"
        spell = stats(stages["spell"])
        r = {"input": name, "n_unitigs": int(g.info()["n_unitigs"]), "bubbles": int(len(bubbles)), "entries": int(len(entries)), "min_block": a.min_block, "sequences": int(len(recs)),
             "bytes": int(len(data)), "longest_sequence": int(recs["length"].max()) if len(recs) else 0, "bad_junctions": bad, "reps": a.reps, "blocks_haplotypes_ms": stats(total), "python_wrapper_ms": stats(wrapper),
             "items_scan_ms": stats(stages["items"]), "spell_ms": spell, "records_ms": stats(stages["records"]),
             "spell_gb_per_s": round(len(data) / spell["median"] / 1e6, 1) if spell["median"] else None, "streaming_copy_gb_per_s": STREAM_COPY_TBS * 1e3,
             "host_numpy_gather_ms": round(host_ms, 1)}
        print(json.dumps(r), flush=True)
        g.close()


if __name__ == "__main__":
    main()
