#!/usr/bin/env python3
"""The three outputs of bgr_align_fasta_text on ONE piece of synthetic FASTA, alternated in one process: want_output 1 (path records), 2 (-c) and 3 (--gaf).

  python tools/gaf_text_bench.py [reads] [reps]        host wall time per call (copies included), bytes out
  rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/gaf_text_bench.py [reads] [reps]
  python tools/gaf_text_bench.py --parse DIR [reads]   device time of each output's launches per piece and per 20 M reads, from that trace
"""
import csv
import glob
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OUT_KERNELS = {1: ("bgr_text_format_kernel",), 2: ("bgr_text_correct_sizes", "bgr_scan2_", "bgr_text_correct_write"), 3: ("bgr_text_gaf_sizes", "bgr_scan2_", "bgr_text_gaf_write")}


def parse(d, n):
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit("no *kernel_trace.csv under " + d)
    rows = []
    for f in files:
        with open(f) as fh:
            for r in csv.DictReader(fh):
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    calls, cur = [], None   # a call = the dispatches from one parse kernel to the next
    for s, e, name in rows:
        if "bgr_text_parse_kernel" in name:
            cur = []
            calls.append(cur)
        if cur is not None:
            cur.append((name, (e - s) / 1e3))
    per = {1: [], 2: [], 3: []}
    parts = {1: {}, 2: {}, 3: {}}
    for c in calls:
        names = " ".join(x for x, _ in c)
        mode = 3 if "bgr_text_gaf" in names else 2 if "bgr_text_correct" in names else 1 if "bgr_text_format" in names else 0
        if not mode:
            continue
        t = 0.0
        for name, us in c:
            for key in OUT_KERNELS[mode]:
                if key in name:
                    t += us
                    parts[mode].setdefault(key, []).append(us)
        per[mode].append(t)
    print("# device time of the output launches behind the mapping launch, one piece of %d reads x 150 bp (us; first call of each output dropped as warm-up)" % n)
    for mode in (1, 2, 3):
        v = per[mode][1:]
        if not v:
            continue
        med = statistics.median(v)
        print("want_output %d: n %d  median %.1f  min %.1f  max %.1f us per piece  -> %.2f ms per 20 M reads" % (mode, len(v), med, min(v), max(v), med * 20e6 / n / 1e3))
        for key, us in parts[mode].items():
            k = len(us) // max(1, len(per[mode]))   # dispatches of this kernel family per call (the scan: three)
            tot = [sum(us[i * k:(i + 1) * k]) for i in range(1, len(per[mode]))]
            print("    %-28s median %.1f us per piece" % (key + "*", statistics.median(tot)))


def main():
    import ctypes as C

    import numpy as np

    import bgreat_amd as B
    from tools.synth import Synth

    n = int(sys.argv[1]) if len(sys.argv) > 1 else 256 * 1024
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 6
    s = Synth(4_600_000, 140, 2, 31, 20261003)
    seqs, offs = s.unitigs()
    g = B.Graph.build(31, seqs, offs)
    al = B.Aligner(g, 0)
    f = os.path.join(os.environ.get("TMPDIR", "/tmp"), "gaf_text_bench.%d.fa" % os.getpid())
    s.write_reads(f, 0, n, 150, 2, 77, threads=16)
    text = np.fromfile(f, dtype=np.uint8)
    os.unlink(f)
    lib = B.lib()

    def pinned(nbytes):
        p = C.c_void_p()
        B._check(lib.bgr_host_alloc(nbytes, C.byref(p)))
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint8)), shape=(nbytes,))

    tin = pinned(len(text) + 64)
    tin[: len(text)] = text
    pout, nout = pinned(2 * len(text)), pinned(len(text) + 64)
    p = B.Params(B.MODE_GREEDY, 2, 2, 0)
    wall = {1: [], 2: [], 3: []}
    out_bytes = {}
    for i in range(reps + 1):   # (round 0: warm-up)
        for want in (1, 2, 3):
            b = B.TextBatch(C.sizeof(B.TextBatch), tin.ctypes.data, len(text), want, 0, pout.ctypes.data, len(pout), nout.ctypes.data, len(nout), 0, 0, 0, 0, None)
            t0 = time.perf_counter()
            B._check(lib.bgr_align_fasta_text(al.h, C.byref(p), C.byref(b)))
            dt = time.perf_counter() - t0
            assert not b.irregular and b.n_accepted == n
            if i:
                wall[want].append(dt * 1e3)
            out_bytes[want] = (int(b.paths_bytes), int(b.notaligned_bytes))
    print("# bgr_align_fasta_text on one piece of %d reads x 150 bp, host wall time per call (copies in and out included), %d calls each, alternated" % (n, reps))
    for want in (1, 2, 3):
        v = wall[want]
        print("want_output %d: median %.2f ms  min %.2f  max %.2f  (%.0f Mreads/s)  paths %d B (%.1f per read)  notAligned %d B" % (
            want, statistics.median(v), min(v), max(v), n / statistics.median(v) / 1e3, out_bytes[want][0], out_bytes[want][0] / n, out_bytes[want][1]))


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--parse":
        parse(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 256 * 1024)
    else:
        main()
