#!/usr/bin/env python3
"""What haplotags cost where they run: bgr_align_fasta_text with want_output 3 (GAF lines) on one piece of 262 144 reads of 150 bp of bench.py's
default Synth shape (genome 4.6 M, spacing 140, 2 alleles, k = 31), with the tag table off and on, and the stand-alone bgr_aligner_haplotags call
over a device-resident launch of the same reads.  The table is built from the graph's own blocks -- the tables of links and triples filled by the
launches tools/blocks_rate.py uses, the bubbles called, phased and chained on the device, then bgr_blocks_tag_table.

Every series is a process of its own (graph built, reads made, one warm-up call, --calls timed calls; host wall time per call, copies in and out
included, into page-locked buffers), and the series alternate: with --parent DIR -- a checkout of the parent commit, built -- each of the --rounds
rounds runs "off" on the parent, "off" on this tree and "on" on this tree in turn; "off on this" against "off on the parent" has to lie inside
the spread of the parent's own rounds, since the untagged kernels are the same code.  One JSON line on stdout:
    python tools/haplotag_rate.py [--parent DIR] [--rounds 5] [--calls 8] [--reads 262144] > profiles/haplotag_rate.txt
(a child: python tools/haplotag_rate.py --child off|on [--root DIR])"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, L = 31, 150


def stats(v):
    return {"median": round(statistics.median(v), 3), "range": [round(min(v), 3), round(max(v), 3)]}


def child(a):
    root = os.path.abspath(a.root) if a.root else HERE
    sys.path.insert(0, root)
    import ctypes as C

    import numpy as np

    import bgreat_amd as B
    from tools.synth import Synth

    assert os.path.dirname(os.path.dirname(os.path.abspath(B.__file__))) == root
    R = a.reads
    syn = Synth(4_600_000, 140, 2, K, 20261003)
    seqs, offs = syn.unitigs()
    g = B.Graph.build(K, seqs, offs)
    n_unitigs = g.info()["n_unitigs"]
    al = B.Aligner(g, 0)
    f = os.path.join(os.environ.get("TMPDIR", "/tmp"), "haplotag_rate.%d.fa" % os.getpid())
    syn.write_reads(f, 0, R, L, 2, 77, threads=16)
    text = np.fromfile(f, dtype=np.uint8)
    os.unlink(f)
    out = {"mode": a.child, "root": os.path.relpath(root, HERE), "reads": R, "n_unitigs": n_unitigs}
    arr, _ = syn.reads(0, R, L, 2, 77, threads=16)
    rd = B.DeviceBuffer(0, arr)
    od = B.DeviceBuffer(0, np.arange(R + 1, dtype=np.uint64) * np.uint64(L))
    if a.child == "on":   # the graph's own blocks, from the rows of ten launches of these reads
        al.links_enable()
        al.triples_enable()
        for _ in range(10):
            al.align_device(rd.data_ptr(), od.data_ptr(), R, R * L, L, m=2, effort=2)
        al.sync()
        bubbles = al.bubbles(1)
        phase = B.bubbles_phase(bubbles, al.triples())
        entries = B.phase_blocks(bubbles, phase, n_unitigs)
        table, n_tagged = B.blocks_tag_table(bubbles, entries, n_unitigs)
        out.update(bubbles=int(len(bubbles)), blocks=int((entries["index"] == 0).sum()), tagged_unitigs=n_tagged, table_bytes=int(table.nbytes))
        al.close()
        al = B.Aligner(g, 0)   # (a fresh one: no counting kernels behind the launches that are timed)
        al.haplotag_enable(table)
    lib = B.lib()

    def pinned(nbytes):
        p = C.c_void_p()
        B._check(lib.bgr_host_alloc(nbytes, C.byref(p)))
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(nbytes,))

    tin = pinned(len(text) + 64)
    tin[: len(text)] = text
    pout, nout = pinned(3 * len(text)), pinned(len(text) + 64)
    p = B.Params(B.MODE_GREEDY, 2, 2, 0)
    wall = []
    for i in range(a.calls + 1):   # (call 0: warm-up)
        b = B.TextBatch(C.sizeof(B.TextBatch), tin.ctypes.data, len(text), 3, 0, pout.ctypes.data, len(pout), nout.ctypes.data, len(nout), 0, 0, 0, 0, None)
        t0 = time.perf_counter()
        B._check(lib.bgr_align_fasta_text(al.h, C.byref(p), C.byref(b)))
        dt = time.perf_counter() - t0
        assert not b.irregular and b.n_accepted == R
        if i:
            wall.append(dt * 1e3)
    out.update(text_call_ms=[round(x, 3) for x in wall], paths_bytes=int(b.paths_bytes))
    if a.child == "on":
        lines = bytes(pout[: int(b.paths_bytes)]).split(b"\n")[:-1]
        out["lines"] = len(lines)
        out["lines_tagged"] = sum(1 for ln in lines if b"\tPS:i:" in ln)
        # the stand-alone call behind a device-resident launch (the launch waited for first: the call is one kernel and one copy)
        alone = []
        for i in range(a.calls + 1):
            al.align_device(rd.data_ptr(), od.data_ptr(), R, R * L, L, m=2, effort=2)
            al.sync()
            t0 = time.perf_counter()
            tags = al.haplotags(R)
            if i:
                alone.append((time.perf_counter() - t0) * 1e3)
        out["haplotags_call_ms"] = [round(x, 3) for x in alone]
        out["reads_tagged"] = int((tags["block"] != 0).sum())
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=["off", "on"])
    ap.add_argument("--root")
    ap.add_argument("--parent", help="a built checkout of the parent commit")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=8)
    ap.add_argument("--reads", type=int, default=262144)
    a = ap.parse_args()
    if a.child:
        return child(a)
    series = ([("parent_off", "off", a.parent)] if a.parent else []) + [("this_off", "off", None), ("this_on", "on", None)]
    got = {name: [] for name, _, _ in series}
    for r in range(a.rounds):
        for name, mode, root in series:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--calls", str(a.calls), "--reads", str(a.reads)] + (["--root", root] if root else [])
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if p.returncode != 0:
                raise SystemExit("%s failed (%d): %s" % (cmd, p.returncode, p.stderr[-2000:]))
            got[name].append(json.loads(p.stdout.strip().split("\n")[-1]))
            print("# round %d %s: median %.3f ms" % (r, name, statistics.median(got[name][-1]["text_call_ms"])), file=sys.stderr, flush=True)
    on = got["this_on"][-1]
    out = {"what": "bgr_align_fasta_text, want_output 3, one piece of %d reads x %d bp, host wall ms per call; %d rounds of %d calls, a process per series, alternated" % (a.reads, L, a.rounds, a.calls)}
    for name in got:
        meds = [statistics.median(x["text_call_ms"]) for x in got[name]]
        out[name + "_ms"] = {"median_of_round_medians": round(statistics.median(meds), 3), "round_medians": [round(m, 3) for m in meds],
                             "all_calls": stats([v for x in got[name] for v in x["text_call_ms"]])}
    out["haplotags_call_ms"] = stats([v for x in got["this_on"] for v in x["haplotags_call_ms"]])
    for key in ("n_unitigs", "bubbles", "blocks", "tagged_unitigs", "table_bytes", "lines", "lines_tagged", "reads_tagged", "paths_bytes"):
        out[key] = on[key]
    out["paths_bytes_untagged"] = got["this_off"][-1]["paths_bytes"]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
