#!/usr/bin/env python3
"""What the cs:Z: field costs where it is made: bgr_align_fasta_text with want_output 3 (GAF lines) on one piece of 262 144 reads of 150 bp of
bench.py's default Synth shape (genome 4.6 M, spacing 140, 2 alleles, k = 31; reads with up to two substitutions), with the field off and on.

Every series is a process of its own (graph built, reads made, one warm-up call, --calls timed calls; host wall time per call around the call's own
device synchronise, copies in and out included, into page-locked buffers), and the series alternate: with --parent DIR -- a checkout of the parent
commit, built -- each of the --rounds rounds runs "off" on the parent, "off" on this tree and "on" on this tree in turn; "off on this" against
"off on the parent" has to lie inside the spread of the parent's own rounds, since the kernels without the field are the same code.  The cost of
"on" is reported next to the growth of the stream in bytes.  One JSON line on stdout:
    python tools/gaf_cs_rate.py [--parent DIR] [--rounds 5] [--calls 8] [--reads 262144] > profiles/gaf_cs_rate.txt
(a child: python tools/gaf_cs_rate.py --child off|on [--root DIR])"""
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
    al = B.Aligner(g, 0)
    f = os.path.join(os.environ.get("TMPDIR", "/tmp"), "gaf_cs_rate.%d.fa" % os.getpid())
    syn.write_reads(f, 0, R, L, 2, 77, threads=16)
    text = np.fromfile(f, dtype=np.uint8)
    os.unlink(f)
    out = {"mode": a.child, "root": os.path.relpath(root, HERE), "reads": R}
    if a.child == "on":
        al.gaf_cs_enable()
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
    lines = bytes(pout[: int(b.paths_bytes)]).split(b"\n")[:-1]
    out.update(text_call_ms=[round(x, 3) for x in wall], paths_bytes=int(b.paths_bytes), lines=len(lines))
    if a.child == "on":
        ops = [ln.rpartition(b"\tcs:Z:")[2] for ln in lines]
        out["lines_with_a_difference"] = sum(1 for o in ops if b"*" in o)
        out["differences"] = sum(o.count(b"*") for o in ops)
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
    on, off = got["this_on"][-1], got["this_off"][-1]
    out = {"what": "bgr_align_fasta_text, want_output 3, one piece of %d reads x %d bp, host wall ms per call; %d rounds of %d calls, a process per series, alternated" % (a.reads, L, a.rounds, a.calls)}
    for name in got:
        meds = [statistics.median(x["text_call_ms"]) for x in got[name]]
        out[name + "_ms"] = {"median_of_round_medians": round(statistics.median(meds), 3), "round_medians": [round(m, 3) for m in meds],
                             "all_calls": stats([v for x in got[name] for v in x["text_call_ms"]])}
    out.update(lines=on["lines"], lines_with_a_difference=on["lines_with_a_difference"], differences=on["differences"], paths_bytes_off=off["paths_bytes"],
               paths_bytes_on=on["paths_bytes"], stream_growth=round(on["paths_bytes"] / off["paths_bytes"] - 1, 4))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
