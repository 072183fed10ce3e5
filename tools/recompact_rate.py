#!/usr/bin/env python3
"""What re-compacting the read-supported graph costs (bgr_graph_recompact), end to end and per stage, with the spell pass in GB/s of written bytes
next to the device's streaming-copy figure, and next to the time tests/recompact_ref.py needs for the same result in plain Python -- a yardstick
for the reader, not a bar.  The input: bench.py's default Synth shape (genome 4.6 M, spacing 140, 2 alleles, k = 31) with keep = (reads >= min_reads)
from the abundance of eleven launches of 262 144 reads, at min_reads 0, 1 and 3.  --reps repetitions taken in turn over the three thresholds; medians
and ranges.  The stages' milliseconds come from HIP events (bgr_graph_recompact_times: ends + successors, ranking, place + scans, spell -- from an
event recorded behind the allocation of the output to one behind the kernel --, records); `recompact_ms` is the whole C call that delivers the
result into buffers of the right size, on the host's clock around it: the upload of the keep bytes, the allocations, the waits, the result's way
back.  One JSON line per threshold on stdout:
    python tools/recompact_rate.py [--min-reads 0,1,3] [--reps 5] [--no-ref] > profiles/recompact_rate.txt"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402

import bgreat_amd as B  # noqa: E402
import recompact_ref  # noqa: E402
from tools.abundance_rate import K, series  # noqa: E402
from tools.bubbles_rate import stats  # noqa: E402
from tools.synth import Synth  # noqa: E402

STREAM_COPY_TBS = 6.29   # the streaming-copy figure the README quotes for one MI355X


def timed_call(g, keep, sizes):
    """the delivering C call alone, into arrays of the sizes a call before it gave -> (ms on the host's clock, records, walk, characters)"""
    out, walk, seq = np.zeros(sizes[0], dtype=B.CHAIN_DTYPE), np.zeros(sizes[1], dtype=np.int32), np.zeros(sizes[2], dtype=np.uint8)
    n, nw, nb = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    t0 = time.perf_counter()
    rc = B.lib().bgr_graph_recompact(g.h, 0, keep.ctypes.data, len(keep), out.ctypes.data, len(out), C.byref(n), walk.ctypes.data, len(walk), C.byref(nw), seq.ctypes.data, len(seq),
                                     C.byref(nb))
    ms = (time.perf_counter() - t0) * 1e3
    assert rc == 0 and (n.value, nw.value, nb.value) == tuple(sizes), (rc, n.value, nw.value, nb.value, sizes)
    return ms, out, walk, seq


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--min-reads", default="0,1,3")
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--reads", type=int, default=262144)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-ref", action="store_true", help="leave out the plain-Python yardstick (and with it the comparison of every byte)")
    a = ap.parse_args()
    t_start = time.perf_counter()
    note = lambda what: print("# %s (%.0f s)" % (what, time.perf_counter() - t_start), file=sys.stderr, flush=True)
    syn = Synth(4_600_000, 140, 2, K, 1234)
    seqs, offs = syn.unitigs()
    R, L = a.reads, 150
    arr, _ = syn.reads(0, R, L, 2, 4321, threads=16)
    g = B.Graph.build(K, seqs, offs)
    note("graph built")
    al = B.Aligner(g, 0)
    al.abundance_enable()
    rd = B.DeviceBuffer(0, arr)
    od = B.DeviceBuffer(0, np.arange(R + 1, dtype=np.uint64) * np.uint64(L))
    series(al, rd, od, R, L, a.launches)   # (one launch to warm up and `launches` more: eleven by default)
    reads_col = np.ascontiguousarray(al.abundance()[:, 0])
    rd.free()
    od.free()
    al.close()
    g.upload(0)
    note("abundance counted")
    mins = [int(x) for x in a.min_reads.split(",")]
    keeps = {m: (reads_col >= m).astype(np.uint8) for m in mins}
    g.recompact(keeps[mins[0]])   # (the first call of a process loads the kernels)
    sizes, whole, got = {}, {m: [] for m in mins}, {}
    stages = {m: {key: [] for key in ("links", "rank", "place", "spell", "records")} for m in mins}
    for m in mins:
        r, w, s = g.recompact(keeps[m])
        sizes[m] = (len(r), len(w), len(s))
    for _ in range(a.reps):   # in turn: a drift of the machine lands on all three alike
        for m in mins:
            ms, out, walk, seq = timed_call(g, keeps[m], sizes[m])
            whole[m].append(ms)
            t = B.recompact_times()
            for key in stages[m]:
                stages[m][key].append(t[key])
            got[m] = (out, walk, seq)
    note("device done")
    unitigs = None
    if not a.no_ref:
        text = bytes(seqs).decode()
        unitigs = [text[int(offs[i]):int(offs[i + 1])] for i in range(len(offs) - 1)]
    for m in mins:
        out, walk, seq = got[m]
        ref_ms = None
        if unitigs is not None:
            t0 = time.perf_counter()
            want = recompact_ref.records(recompact_ref.compact(unitigs, keeps[m].tolist(), K, check=False))
            ref_ms = round((time.perf_counter() - t0) * 1e3, 1)
            assert [tuple(int(x) for x in row) for row in out] == want[0] and walk.tolist() == want[1] and seq.tobytes() == want[2], "the device and recompact_ref.py disagree"
            note("min_reads %d checked against recompact_ref.py" % m)
        spell = stats(stages[m]["spell"])
        r = {"input": "default", "n_unitigs": int(g.info()["n_unitigs"]), "min_reads": m, "kept": int(keeps[m].sum()), "chains": int(len(out)), "circular": int((out["flags"] & 1).sum()),
             "longest_walk": int(out["n_unitigs"].max()) if len(out) else 0, "bytes": int(len(seq)), "reps": a.reps, "recompact_ms": stats(whole[m]), "ends_succ_ms": stats(stages[m]["links"]),
             "rank_ms": stats(stages[m]["rank"]), "place_scans_ms": stats(stages[m]["place"]), "spell_ms": spell, "records_ms": stats(stages[m]["records"]),
             "spell_gb_per_s": round(len(seq) / spell["median"] / 1e6, 1) if spell["median"] else None, "streaming_copy_gb_per_s": STREAM_COPY_TBS * 1e3, "recompact_ref_py_ms": ref_ms}
        print(json.dumps(r), flush=True)
    g.close()


if __name__ == "__main__":
    main()
