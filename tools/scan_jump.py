#!/usr/bin/env python3
"""A CPU model of the jump in front of the greedy multi kernel's anchor scan (no GPU; greedy_kernels.hip, graph_layout.h: jump index), in the
style of tools/scan_halves.py, from bench.py's seeded reads.  The index holds one (k-1)-mer in --stride of every unitig, chosen by a hash of its canonical form
(canonical form -> unitig, offset, strand; palindromes left out; a share --drop of the entries is lost, as the two-entry buckets of the real
table lose them).  An item hashes its first --probes windows and probes the index once, with the first window the hash selects (--by-offset:
the index holds every --stride-th offset instead and all --probes windows are probed -- the first scheme tried; it costs --probes loads per
item where the hash scheme costs one); a hit names a diagonal, the read is compared with the unitig along
it from the item's first position to the first mismatch, and the windows of that stretch are keys exactly where the diagonal passes a unitig
end (property P, checked here as the builder checks it).  The item is then settled (its first anchor, or none), or its scan starts behind the
stretch, or -- no hit, or a stretch that starts behind the item's first position -- it is scanned as before.  The model asserts that a
settled item's answer is the plain scan's first anchor and that no raised start skips one.  Printed: the share of items settled, of items
whose start was raised, and the steps of two 32-lane scanners per sixteen items before and after (a scanner starts at the item's start rounded
down to 16).  Items: the forward first items, and with them the reverse-complement items of the reads the oracle marks (status bit 2).
The defaults are bench.py's default workload (configs[2]); configs[1]:  python tools/scan_jump.py --genome 250000 --site-spacing 75 --read-len 100
tools/scan_steps.py on the diagnostic build is the measured counterpart."""
import argparse
import os
import random
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from tools.synth import Synth  # noqa: E402
import oracle_py  # noqa: E402

ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
ap.add_argument("--reads", type=int, default=65536)
ap.add_argument("--genome", type=int, default=4_600_000)
ap.add_argument("--site-spacing", type=int, default=140)
ap.add_argument("--alleles", type=int, default=2)
ap.add_argument("--read-len", type=int, default=150)
ap.add_argument("--k", type=int, default=31)
ap.add_argument("--mismatch", type=int, default=2)
ap.add_argument("--seed-graph", type=int, default=20261003)
ap.add_argument("--seed-reads", type=int, default=77)
ap.add_argument("--stride", type=int, default=4)
ap.add_argument("--probes", type=int, default=12, help="windows of an item that are looked at (the kernel: 4 x BGR_JUMP_WINDOWS)")
ap.add_argument("--by-offset", action="store_true", help="sample every --stride-th offset and probe every window (use --probes 4)")
ap.add_argument("--drop", type=float, default=0.10, help="share of the sampled (k-1)-mers that the table loses")
a = ap.parse_args()
K1, N, Lr = a.k - 1, a.reads, a.read_len
npos = Lr - K1 + 1

syn = Synth(a.genome, a.site_spacing, a.alleles, a.k, a.seed_graph)
seqs, offs = syn.unitigs()
reads, _ = syn.reads(0, N, Lr, a.mismatch, a.seed_reads)
S, R = bytes(seqs), bytes(reads)
tr = bytes.maketrans(b"ACGT", b"TGCA")


def rc(x):
    return x.translate(tr)[::-1]


U = [S[int(offs[i]):int(offs[i + 1])] for i in range(len(offs) - 1)]
URC = [rc(u) for u in U]
J = set()
for u in U:
    for x in (u[:K1], u[len(u) - K1:]):
        J.add(x)
        J.add(rc(x))
# property P
for u in U:
    for t in range(1, len(u) - K1):
        assert u[t:t + K1] not in J, "an interior (k-1)-mer of a unitig is an overlap key: no index for this graph"
rng = random.Random(1)
index = {}
n_sampled = 0


def selects(canon):
    return zlib.crc32(canon) % a.stride == 0


for i, u in enumerate(U):
    for t in range(0, len(u) - K1 + 1, a.stride if a.by_offset else 1):
        w = u[t:t + K1]
        r = rc(w)
        if w == r or not (a.by_offset or selects(min(w, r))):
            continue
        n_sampled += 1
        if rng.random() < a.drop:
            continue
        index.setdefault(min(w, r), (i, t, w < r))
print("unitigs %d, sampled (k-1)-mers %d, entries %d (%.1f MB at 8 B per entry, one 16-byte bucket per sample)" % (len(U), n_sampled, len(index), 16 * n_sampled / 1e6))


def first_anchor(r, start=0):
    return next((j for j in range(start, npos) if r[j:j + K1] in J), -1)


def jump(r, g_from=0):
    """-> ('settled', anchor or -1) | ('raised', new start) | ('scan', g_from)"""
    for sub in range(a.probes):
        p = g_from + sub
        if p >= npos:
            break
        w = r[p:p + K1]
        c = rc(w)
        if not a.by_offset and (w == c or not selects(min(w, c))):
            continue
        e = index.get(min(w, c))
        if e is None:
            if a.by_offset:
                continue
            return ("scan", g_from)                 # one probe per item
        i, t, fwd_canon = e
        rcs = (w <= c) != fwd_canon                 # the read runs along the unitig's other strand
        ulen = len(U[i])
        u = ulen - K1 - t if rcs else t             # the probed window's offset on that strand
        if u < sub:
            return ("scan", g_from)                 # the stretch would start behind the item's first position
        u0 = u - sub
        strand = URC[i] if rcs else U[i]
        hi = min(Lr, g_from + ulen - u0)
        e_pos = next((q for q in range(g_from, hi) if r[q] != strand[u0 + q - g_from]), hi)
        last = e_pos - K1
        if last < g_from:
            return ("scan", g_from)
        p1 = g_from + (ulen - K1 - u0)
        if u0 == 0:
            return ("settled", g_from)
        if p1 <= last and p1 < npos:
            return ("settled", p1)
        if last >= npos - 1:
            return ("settled", -1)
        return ("raised", last + 1)
    return ("scan", g_from)


def scan_steps(start, anchor):  # steps of a 32-lane scanner that starts at `start` rounded down to 16
    hb = start & ~15
    return (anchor - hb) // 32 + 1 if anchor >= 0 else (npos - hb + 31) // 32


def wave_steps(st):  # list scheduling of one wave's items, in order, on two scanners
    free = [0, 0]
    for s in st:
        j = 0 if free[0] <= free[1] else 1
        free[j] += int(s)
    return max(free)


def model(items, label):
    before, after, settled, raised = [], [], 0, 0
    for r in items:
        fa = first_anchor(r)
        what, v = jump(r)
        before.append(scan_steps(0, fa))
        if what == "settled":
            assert v == fa, "the jump's answer differs from the plain scan's first anchor"
            settled += 1
            after.append(0)
        else:
            assert first_anchor(r, v) == fa, "a raised start skipped an anchor"
            raised += what == "raised"
            after.append(scan_steps(v, fa))
    W = len(items) // 16
    b = np.mean([wave_steps(before[w * 16:(w + 1) * 16]) for w in range(W)])
    f = np.mean([wave_steps(after[w * 16:(w + 1) * 16]) for w in range(W)])
    print("%s: %d items, settled without a scan step %.1f %%, start raised %.1f %%; steps per sixteen items %.2f -> %.2f" % (
        label, len(items), 100 * settled / len(items), 100 * raised / len(items), b, f))


fw = [R[i * Lr:(i + 1) * Lr] for i in range(N)]
_, _, status = oracle_py.Oracle(a.k, seqs, offs).align(reads, np.arange(N + 1, dtype=np.uint64) * np.uint64(Lr), m=a.mismatch, effort=2)
model(fw, "first items")
model(fw + [rc(fw[i]) for i in np.nonzero(status & 4)[0]], "first + reverse-complement items")
