#!/usr/bin/env python3
"""A CPU model of the greedy multi kernel's anchor-scan steps per sixteen reads (no GPU): one 64-lane scanner against two 32-lane (and four
16-lane) scanners, from bench.py's seeded reads.  A read's first anchor = its first (k-1)-mer that starts or ends a unitig (a key of the
table, either orientation); a scanner of w lanes is done with a read at the step that holds its first anchor, ceil((a + 1) / w) steps, or
once it has passed the read's npos = L - k + 2 positions, ceil(npos / w) steps.  Several scanners take the wave's sixteen reads in order,
each the next one as soon as it is free (the lowest scanner first); the steps of a wave = until all are idle.  Only first items (the forward
strand from position 0) are counted in the first figures; a second set adds, through the oracle, the reverse-complement item of every read
whose forward anchors all failed or that had none (status bit 2), as items of their own behind the first ones, sixteen to a wave.  Follow-up
items of the same strand (a second anchor) are left out, so both sets are lower bounds on the kernel's steps (tools/scan_steps.py measures them).
The defaults are bench.py's default workload (configs[2]); pass bench.py's values for another one, e.g. configs[1]:
    python tools/scan_halves.py --genome 250000 --site-spacing 75 --read-len 100"""
import argparse
import os
import sys

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
a = ap.parse_args()
K1, N, Lr = a.k - 1, a.reads, a.read_len
npos = Lr - K1 + 1

syn = Synth(a.genome, a.site_spacing, a.alleles, a.k, a.seed_graph)
seqs, offs = syn.unitigs()
reads, _ = syn.reads(0, N, Lr, a.mismatch, a.seed_reads)
S, R = bytes(seqs), bytes(reads)
tr = bytes.maketrans(b"ACGT", b"TGCA")
J = set()
for i in range(len(offs) - 1):
    lo, hi = int(offs[i]), int(offs[i + 1])
    for x in (S[lo:lo + K1], S[hi - K1:hi]):
        J.add(x)
        J.add(x.translate(tr)[::-1])


def first_anchor(r):
    return next((j for j in range(npos) if r[j:j + K1] in J), -1)


first = np.array([first_anchor(R[i * Lr:(i + 1) * Lr]) for i in range(N)], dtype=np.int64)
_, _, status = oracle_py.Oracle(a.k, seqs, offs).align(reads, np.arange(N + 1, dtype=np.uint64) * np.uint64(Lr), m=a.mismatch, effort=2)
rc_first = np.array([first_anchor(R[i * Lr:(i + 1) * Lr].translate(tr)[::-1]) for i in np.nonzero(status & 4)[0]], dtype=np.int64)


def steps(a_pos, lanes):  # steps one scanner of `lanes` lanes spends on each read
    return np.where(a_pos >= 0, a_pos // lanes + 1, (npos + lanes - 1) // lanes)


def wave_steps(st, n_scan):  # list scheduling of one wave's reads, in order, on n_scan scanners
    free = [0] * n_scan
    for s in st:
        j = min(range(n_scan), key=lambda x: (free[x], x))
        free[j] += int(s)
    return max(free)


have = first >= 0
print("reads %d, read length %d, npos %d; first anchor: none %.1f %%, before 18 %.1f %%, before 32 %.1f %%, before 64 %.1f %%"
      % (N, Lr, npos, 100 * np.mean(~have), 100 * np.mean(have & (first < 18)), 100 * np.mean(have & (first < 32)), 100 * np.mean(have & (first < 64))))
print("reverse-complement items (oracle status bit 2): %d (%.1f %% of the reads)" % (len(rc_first), 100 * len(rc_first) / N))


def model(items, label):
    W = len(items) // 16
    for n_scan in (1, 2, 4):
        lanes = 64 // n_scan
        st = steps(items, lanes)
        per_wave = [wave_steps(st[w * 16:(w + 1) * 16], n_scan) for w in range(W)]
        print("%s: %d scanner%s x %2d lanes: %.2f steps per sixteen items, %.3f per read" % (
            label, n_scan, "" if n_scan == 1 else "s", lanes, np.mean(per_wave), np.sum(per_wave) / N))
    need = np.where(items >= 0, items + 1, npos)
    print("%s: ideal (positions needed / 64 per wave): %.2f" % (label, np.mean([-(-int(need[w * 16:(w + 1) * 16].sum()) // 64) for w in range(W)])))


model(first, "first items")
model(np.concatenate([first, rc_first]), "first + reverse-complement items")
