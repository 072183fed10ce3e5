#!/usr/bin/env python3
"""A CPU model of the greedy walk's steps per side, and of walk-loop iterations per sixteen reads (no GPU): seeded synthetic reads through
the oracle.  The anchor of a read = its first (k-1)-mer that starts or ends a unitig (the keys of the table); its left / right steps = the
path's unitigs before / after it.  Only forward-strand first items that align are counted (every other item as 0 steps), so the iteration
figures are lower bounds; sixteen reads per wave in input order, as the multi kernel takes them.
The defaults are bench.py's default workload (configs[2]); pass bench.py's values for another one, e.g. configs[1]:
    python tools/walk_sides.py --genome 250000 --site-spacing 75 --read-len 100"""
import argparse
import collections
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
ap.add_argument("--effort", type=int, default=2)
ap.add_argument("--seed-graph", type=int, default=20261003)
ap.add_argument("--seed-reads", type=int, default=77)
a = ap.parse_args()
K1, N, Lr = a.k - 1, a.reads, a.read_len

syn = Synth(a.genome, a.site_spacing, a.alleles, a.k, a.seed_graph)
seqs, offs = syn.unitigs()
reads, roffs = syn.reads(0, N, Lr, a.mismatch, a.seed_reads)
o = oracle_py.Oracle(a.k, seqs, offs)
p, po, st = o.align(reads, roffs, m=a.mismatch, effort=a.effort)
S, R = bytes(seqs), bytes(reads)
tr = bytes.maketrans(b"ACGT", b"TGCA")
ulen = np.diff(offs.astype(np.int64))
J = set()
for i in range(len(offs) - 1):
    lo, hi = int(offs[i]), int(offs[i + 1])
    for x in (S[lo:lo + K1], S[hi - K1:hi]):
        J.add(x)
        J.add(x.translate(tr)[::-1])
LR, off_path, no_junction = [], 0, 0
for i in range(N):
    if st[i] != 2:  # aligned on the forward strand
        LR.append(None)
        continue
    r = R[i * Lr:(i + 1) * Lr]
    anc = next((j for j in range(Lr - K1 + 1) if r[j:j + K1] in J), None)
    if anc is None:
        no_junction += 1
        LR.append(None)
        continue
    path = p[po[i]:po[i + 1]]
    off, us = int(path[0]), [abs(int(x)) - 1 for x in path[1:]]
    if anc == 0:
        LR.append((0, len(us)))
        continue
    P, x = [], ulen[us[0]] - K1 - off
    P.append(x)
    for u in us[1:]:
        x += ulen[u] - K1
        P.append(x)
    if anc not in P:
        off_path += 1
    nl = sum(1 for q in P if q <= anc)
    LR.append((nl, len(us) - nl))
ok = [x for x in LR if x]
print("reads", N, "forward-aligned", len(ok), "anchor not at a junction of the path:", off_path, "no junction found:", no_junction)
print("left steps", sorted(collections.Counter(x[0] for x in ok).items()))
print("right steps", sorted(collections.Counter(x[1] for x in ok).items()))
print("mean left %.2f right %.2f" % (np.mean([x[0] for x in ok]), np.mean([x[1] for x in ok])))
seq_it, par_it = [], []
for w in range(0, N - 15, 16):
    grp = [x or (0, 0) for x in LR[w:w + 16]]
    seq_it.append(max(l + r for l, r in grp))
    par_it.append(max(max(l, r) for l, r in grp))
print("walk-loop iterations per 16 reads (model, lower bound): left then right %.2f, both sides at once %.2f" % (np.mean(seq_it), np.mean(par_it)))
