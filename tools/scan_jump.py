#!/usr/bin/env python3
"""A CPU model of the jump in front of the greedy multi kernel's anchor scan (no GPU; greedy_kernels.hip, graph_layout.h: jump index), in the
style of tools/scan_halves.py, from bench.py's seeded reads.  The index holds one (k-1)-mer in --stride of every unitig, chosen by a hash of its canonical form
(canonical form -> unitig, offset, strand; palindromes left out; a share --drop of the entries is lost, as the two-entry buckets of the real
table lose them).  An item hashes its first --near windows and --far windows from --far-offset on (default: --near + k-1, so that they share
no base with the near ones) and probes the index with the first window of either set that the hash selects; the near entry is used when
it hits, else the far one.  A hit names a diagonal: the strand occupies read positions [A, A + len), and the read is compared with it over
[max(A, start), min(A + len, L)), past --past mismatches (-1, the kernel: past all of them, keeping the first and the last; n >= 0: the
mismatch number n + 1 cuts the stretch, and the verified windows between two mismatches count as well).  A window is verified iff all its k-1 bases
lie in the stretch and none is a mismatch; a verified window is a key exactly where the diagonal passes a unitig end (property P, checked here
as the builder checks it).  fb = the smallest verified key position; the item's scan is left the range from its first unverified window to one
past the last unverified window below fb (below npos without one); an empty range settles the item.  The model asserts for every item that
the range's first key -- fb without one -- is the plain scan's first anchor.  Printed: the share of items settled (and by the far entry),
of items left a bounded range, and the steps of two 32-lane scanners per sixteen items before and after (a scanner starts at the range's start
rounded down to 16).  Items: the forward first items, and with them the reverse-complement items of the reads the oracle marks (status bit 2).
The defaults are the kernel's constants and bench.py's default workload (configs[2]); configs[1]:
python tools/scan_jump.py --genome 250000 --site-spacing 75 --read-len 100.  The scheme before the far probe: --near 12 --far 0 --past 0.
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
ap.add_argument("--near", type=int, default=8, help="near windows of an item that are hashed (BGR_JUMP_NEAR)")
ap.add_argument("--far", type=int, default=4, help="far windows of an item that are hashed (BGR_JUMP_FAR)")
ap.add_argument("--far-offset", type=int, default=-1, help="the first far window, counted from the item's first position (default: near + k-1)")
ap.add_argument("--past", type=int, default=-1, help="mismatches the compare goes past (-1: all, the kernel)")
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
    for t in range(0, len(u) - K1 + 1):
        w = u[t:t + K1]
        r = rc(w)
        if w == r or not selects(min(w, r)):
            continue
        n_sampled += 1
        if rng.random() < a.drop:
            continue
        index.setdefault(min(w, r), (i, t, w < r))
print("unitigs %d, sampled (k-1)-mers %d, entries %d (%.1f MB at 8 B per entry, one 16-byte bucket per sample)" % (len(U), n_sampled, len(index), 16 * n_sampled / 1e6))


FAR0 = a.far_offset if a.far_offset >= 0 else a.near + K1


def first_key(r, lo, hi):
    return next((j for j in range(lo, hi) if r[j:j + K1] in J), -1)


def probe(r, g_from, rels):
    """the first window of `rels` (offsets from g_from) that the hash selects -> (offset, entry or None) | None"""
    for rel in rels:
        p = g_from + rel
        if p >= npos:
            break
        w = r[p:p + K1]
        c = rc(w)
        if w == c or not selects(min(w, c)):
            continue
        return rel, w <= c, index.get(min(w, c))
    return None


def jump(r, g_from=0):
    """-> (lo, hi, fb, by_far): the range left to the scan, the fallback anchor (-1: none), whether the far entry was used"""
    near = probe(r, g_from, range(a.near))
    far = probe(r, g_from, range(FAR0, FAR0 + a.far))
    by_far = not (near and near[2])
    hit = far if by_far else near
    if not hit or not hit[2]:
        return g_from, npos, -1, False
    rel, w_canon, (i, t, fwd_canon) = hit
    rcs = w_canon != fwd_canon                      # the read runs along the unitig's other strand
    ulen = len(U[i])
    u = ulen - K1 - t if rcs else t                 # the probed window's offset on that strand
    strand = URC[i] if rcs else U[i]
    A = g_from + rel - u                            # the strand occupies read positions [A, A + ulen)
    cs, ce = max(A, g_from), min(A + ulen, Lr)
    mis = [q for q in range(cs, ce) if r[q] != strand[q - A]]
    between = []                                    # verified windows between two mismatches (the kernel keeps none)
    if a.past >= 0:
        if len(mis) > a.past:
            ce, mis = mis[a.past], mis[:a.past]
        between = [(mis[n] + 1, mis[n + 1] - K1) for n in range(len(mis) - 1)]
    e1, eL = (mis[0], mis[-1]) if mis else (ce, -1)

    def verified(j):
        return cs <= j and j + K1 <= ce and (j + K1 <= e1 or j > eL or any(x <= j <= y for x, y in between))
    fb = -1
    p1 = A + ulen - K1
    if A >= g_from and A < npos and verified(A):
        fb = A
    elif p1 >= g_from and p1 < npos and verified(p1):
        fb = p1
    lim = fb if fb >= 0 else npos
    lo = next((j for j in range(g_from, lim) if not verified(j)), lim)
    hi = next((j + 1 for j in range(lim - 1, lo - 1, -1) if not verified(j)), lo)
    return lo, hi, fb, by_far


def scan_steps(start, anchor, end):  # steps of a 32-lane scanner that starts at `start` rounded down to 16 and covers [start, end)
    hb = start & ~15
    return (anchor - hb) // 32 + 1 if anchor >= 0 else (end - hb + 31) // 32


def wave_steps(st):  # list scheduling of one wave's items, in order, on two scanners
    free = [0, 0]
    for s in st:
        j = 0 if free[0] <= free[1] else 1
        free[j] += int(s)
    return max(free)


def model(items, label):
    before, after, settled, far_settled, bounded, raised = [], [], 0, 0, 0, 0
    for r in items:
        fa = first_key(r, 0, npos)
        lo, hi, fb, by_far = jump(r)
        h = first_key(r, lo, hi)
        assert (h if h >= 0 else fb) == fa, "range + fallback differ from the plain scan's first anchor"
        before.append(scan_steps(0, fa, npos))
        if lo >= hi:
            settled += 1
            far_settled += by_far
            after.append(0)
        else:
            raised += lo > 0
            bounded += lo > 0 or hi < npos
            after.append(scan_steps(lo, h, hi))
    W = len(items) // 16
    b = np.mean([wave_steps(before[w * 16:(w + 1) * 16]) for w in range(W)])
    f = np.mean([wave_steps(after[w * 16:(w + 1) * 16]) for w in range(W)])
    n = len(items)
    print("%s: %d items, settled without a scan step %.1f %% (by the far entry %.1f %%), scanned a bounded range %.1f %% (start raised %.1f %%); "
          "steps per sixteen items %.2f -> %.2f" % (label, n, 100 * settled / n, 100 * far_settled / n, 100 * bounded / n, 100 * raised / n, b, f))


fw = [R[i * Lr:(i + 1) * Lr] for i in range(N)]
_, _, status = oracle_py.Oracle(a.k, seqs, offs).align(reads, np.arange(N + 1, dtype=np.uint64) * np.uint64(Lr), m=a.mismatch, effort=2)
model(fw, "first items")
model(fw + [rc(fw[i]) for i in np.nonzero(status & 4)[0]], "first + reverse-complement items")
