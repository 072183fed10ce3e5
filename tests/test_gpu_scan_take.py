"""The word a scanner half fetches when it takes an item (bgreat_amd/csrc/scan_take_word.h), against the oracle, row by row.

With the key table in LDS the anchor scan of the sixteen-reads-per-wave greedy kernel packs what a half needs of an item into one word per
group -- resume position (9 bits), positions left (9), the item's dword counted from the wave's first read word (9), 16 - resume position
% 16 (5) -- and a half fetches it with one lane read.  The sets here are the smallest at which a field can be too narrow or an address
wrong:
  - long reads, late anchors: reads of 400-479 bases (sixteen words per read, the most the kernel takes) at k = 31 and k = 12.  A decoy
    unitig ends in a (k-1)-mer taken from inside the read's locus, at a position a >= 256: the read's first anchor lies there and fails
    (nothing continues the decoy), and the follow-up item resumes at a + 1 > 256 and finds the locus's own junction behind it, which maps
    the read (kind "second"); with two decoys the third anchor maps it ("third"); with no junction behind the decoy the read goes on to
    its reverse complement ("rc").  A decoy at a < 48 leaves a follow-up item with more than 256 positions left.  Fresh items have all
    of npos > 256 left.  A batch of such reads alone, in input order, fills every group of a wave with them, fresh (first and last group:
    dword 0 and 15 x 32) and as follow-up items (a full group of sixteen off the wave's queue: dword 15 x 32 + (a + 1) / 16);
  - every residue: a + 1 takes every value mod 16 among the late decoys (the 5-bit field, 16 included);
  - short reads, small k: k = 12 and k = 5, reads of k .. k + 40 bases (two and three words per read: the smallest LDS region of a wave), in
    batches of 1, 15, 17 and 16 n + 7 reads (idle halves, a sparse last group);
  - mixed lengths: a read of ~470 bases without any anchor (a half scans it for fifteen steps) in a wave of reads of k .. k + 9 bases (the
    other half runs out of items and idles), and the long reads above between short ones.
Every set at effort 0-3, m = 2, each read together with its reverse complement, through packed planes (Aligner.align) and ASCII reads
parked on the device (align_device + fetch), with the key table in LDS and in L2, and through the general kernel (KNOB_GREEDY_FAST), whose
rows must be the same: test_gpu_second_anchor.py's _Case.check.  The picker asserts that every bucket holds a read; a host-only test runs it
without a GPU."""
import numpy as np
import pytest

import bgreat_amd as B
import oracle_py
from tools.synth import Synth
from test_gpu_scan_halves import COMP, _pack
from test_gpu_second_anchor import FWD, _Case, _Picked, _anchors, _keys, _kind

SEED = 1201
LONG_KS = (31, 12)
LMIN, LMAX = 400, 479
# (what the decoys do, which anchor of the forward strand maps the read): the buckets of a long set, each with the residues of a + 1 it must show
LONG_BUCKETS = [("late", "second", r) for r in range(16)] + [("early", "second", r) for r in (0, 7, 15)] + \
               [("late2", "third", r) for r in (0, 9)] + [("only", "rc", r) for r in (0, 12)]
PER_BUCKET = 2


def _rand(rng, n):
    return bytes(b"ACGT"[c] for c in rng.integers(0, 4, size=n))


def _rc(r):
    return r.translate(COMP)[::-1]


def _concat(units):
    offs = np.zeros(len(units) + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(u) for u in units])
    return np.frombuffer(b"".join(units), dtype=np.uint8), offs


_LONG = {}


def _pick_long(k):
    """a graph with a junction every ~600 bases plus the decoys, its oracle and {bucket: [reads]} (once per run)"""
    if k in _LONG:
        return _LONG[k]
    k1 = k - 1
    s = Synth(400000, 600, 2, k, SEED + k)
    seqs, offs = s.unitigs()
    J0 = _keys(seqs, offs, k1)
    n = 1500 if k == 31 else 6000
    base, boffs = s.reads(0, n, LMAX, 0, SEED + 2)
    rng = np.random.default_rng(SEED + k)
    plans, decoys = [], []
    need = {b: (3 if k == 31 else 12) for b in LONG_BUCKETS}  # candidates per bucket (k = 12: chance 11-mers spoil some)
    lengths = [LMAX, LMIN]
    for i in range(n):
        r = bytes(base[int(boffs[i]):int(boffs[i + 1])])
        A = _anchors(r, J0, k1)
        open_b = [b for b in LONG_BUCKETS if need[b] and ((b[0] == "only") == (not A))]
        if not open_b or (A and not (300 <= A[0] <= LMIN - k1)):
            continue
        bk = open_b[int(rng.integers(len(open_b)))]
        what, kind, res = bk
        top = A[0] if A else LMIN - k1
        if what == "early":
            cand = [a for a in range(2, 48) if (a + 1) % 16 == res]
        else:
            cand = [a for a in range(256, top - 1) if (a + 1) % 16 == res]
        if not cand:
            continue
        at = [cand[int(rng.integers(len(cand)))]]
        if what == "late2":
            more = [a for a in range(at[0] + 1, top)]
            if not more:
                continue
            at.append(more[int(rng.integers(len(more)))])
        L = lengths.pop() if lengths else int(rng.integers(LMIN, LMAX + 1))
        plans.append((bk, r[:L], at + A))
        decoys += [_rand(rng, 40) + r[a:a + k1] for a in at]
        need[bk] -= 1
    p = _Picked()
    p.k = k
    units = [bytes(seqs[int(offs[i]):int(offs[i + 1])]) for i in range(len(offs) - 1)] + decoys
    p.seqs, p.offs = _concat(units)
    p.o = oracle_py.Oracle(k, p.seqs, p.offs)
    p.J = _keys(p.seqs, p.offs, k1)
    # keep the reads whose anchors are exactly the planned ones (a cut may drop a later junction: a prefix must match) and whose outcome
    # is the bucket's kind
    good = [(bk, r, at) for bk, r, at in plans if _anchors(r, p.J, k1) == [a for a in at if a + k1 <= len(r)]]
    reads, roffs = _pack([r for _, r, _ in good], with_rc=False)
    x = [p.o.align(reads, roffs, m=2, effort=e)[2].tolist() for e in (1, 2, 3)]
    p.by = {b: [] for b in LONG_BUCKETS}
    for (bk, r, at), x1, x2, x3 in zip(good, *x):
        if _kind(x1, x2, x3) == bk[1] and len(p.by[bk]) < PER_BUCKET:
            p.by[bk].append(r)
    empty = [b for b, lst in p.by.items() if not lst]
    assert not empty, (k, empty)  # a condition on the seeds, not a tolerance
    p.reads = [r for b in LONG_BUCKETS for r in p.by[b]]
    p.noanchor = []
    while len(p.noanchor) < 4:  # ~470 random bases without a key: a half scans all of them
        r = _rand(rng, int(rng.integers(465, LMAX + 1)))
        if not _anchors(r, p.J, k1) and not _anchors(_rc(r), p.J, k1):
            p.noanchor.append(r)
    _LONG[k] = p
    return p


@pytest.mark.parametrize("k", LONG_KS)
def test_long_reads_are_what_they_claim(k):
    """(no GPU) every bucket is filled; the late decoys put the first anchor at a >= 256 with a + 1 at every residue, the follow-up item's
    positions left are below 256 there and above 256 behind an early decoy, and the reads are 400-479 bases long, both ends included"""
    p = _pick_long(k)
    k1 = k - 1
    seen = set()
    for (what, kind, res), lst in p.by.items():
        assert 1 <= len(lst) <= PER_BUCKET
        for r in lst:
            assert LMIN <= len(r) <= LMAX
            A = _anchors(r, p.J, k1)
            npos = len(r) - k1 + 1
            assert npos >= 256 and (A[0] + 1) % 16 == res
            if what == "early":
                assert A[0] < 48 and npos - (A[0] + 1) >= 256
            else:
                assert A[0] >= 256
                if what == "late":
                    seen.add((A[0] + 1) % 16)
            assert len(A) == 1 if what == "only" else len(A) >= (3 if what == "late2" else 2)
    assert seen == set(range(16))
    assert {len(r) for r in p.reads} >= {LMIN, LMAX}
    assert len(p.reads) < 400
    # sixteen words per read: the longest read fills fifteen
    assert (max(len(r) for r in p.reads) + 31) // 32 == 15


class _TakeCase(_Case):
    """_Case (three aligners, the oracle's rows per read set and effort) over a graph made here"""

    def __init__(self, p):
        self.p = p
        g = B.Graph.build(p.k, p.seqs, p.offs)
        self.lds, self.l2, self.gen = B.Aligner(g, 0), B.Aligner(g, 0), B.Aligner(g, 0)
        self.lds.configure(lds_mphf=2)
        self.l2.configure(lds_mphf=1)
        self.gen.set_knob(B.KNOB_GREEDY_FAST, 1)
        self.want = {}


_CASES = {}


def _case(key, make):
    if key not in _CASES:
        _CASES[key] = _TakeCase(make())
    return _CASES[key]


@pytest.mark.gpu
@pytest.mark.parametrize("k", LONG_KS)
def test_long_reads_late_anchors(k):
    c = _case(("long", k), lambda: _pick_long(k))
    # the long reads alone, in input order: every group of a wave holds one, fresh and again as a follow-up item off the wave's queue
    late = [r for b in LONG_BUCKETS if b[0] != "early" for r in c.p.by[b]]
    late = (late * (32 // len(late) + 1))[:32] + late[:7]
    c.check("late", *_pack(late, with_rc=False))
    c.check("all", *_pack(c.p.reads))
    # said once more on the rows that matter: effort 2 maps the "second" reads forward, effort 3 the "third" ones
    for kind, effort in (("second", 2), ("third", 3)):
        lst = [r for b in LONG_BUCKETS if b[1] == kind for r in c.p.by[b]]
        for al in (c.lds, c.l2):
            _, _, st = al.align(*_pack(lst, with_rc=False), m=2, effort=effort)
            assert (st == FWD).all(), (kind, effort)


@pytest.mark.gpu
@pytest.mark.parametrize("k", LONG_KS)
def test_mixed_lengths_in_one_wave(k):
    c = _case(("long", k), lambda: _pick_long(k))
    rng = np.random.default_rng(SEED + 7 * k)
    shorts = [r[o:o + int(rng.integers(k, k + 10))] for r in c.p.reads for o in (0, 100, 200, 300)]
    reads = []
    for j, r in enumerate(c.p.noanchor + c.p.reads[:12]):
        at = (0, 15, 7, 1)[j % 4]  # the long read's group in its wave: first, last, in between
        wave = [shorts[(16 * j + q) % len(shorts)] for q in range(15)]
        reads += wave[:at] + [r] + wave[at:]
    c.check("mixed", *_pack(reads, with_rc=False))
    c.check("mixed rc", *_pack([_rc(r) for r in reads], with_rc=False), efforts=(2,))


# ---- short reads, small k ------------------------------------------------------------------------------------------------------------

#          k: (genome, site spacing)
SHORT = {12: (60000, 25), 5: (3000, 25)}
_SHORT = {}


def _pick_short(k):
    if k in _SHORT:
        return _SHORT[k]
    G, d = SHORT[k]
    p = _Picked()
    p.k = k
    s = Synth(G, d, 2, k, SEED + 100 + k)
    p.seqs, p.offs = s.unitigs()
    p.o = oracle_py.Oracle(k, p.seqs, p.offs)
    p.J = _keys(p.seqs, p.offs, k - 1)
    base, boffs = s.reads(0, 16 * 14 + 7, k + 40, 2, SEED + 3)
    rng = np.random.default_rng(SEED + k)
    p.reads = []
    for i in range(len(boffs) - 1):
        r = bytes(base[int(boffs[i]):int(boffs[i + 1])])
        p.reads.append(r[:(k, k + 40, k + 1, k + 20)[i] if i < 4 else int(rng.integers(k, k + 41))])
    _SHORT[k] = p
    return p


@pytest.mark.parametrize("k", sorted(SHORT))
def test_short_reads_are_what_they_claim(k):
    """(no GPU) reads of k .. k + 40 bases, both ends included: two and three words per read; some with an anchor, some that fail one"""
    p = _pick_short(k)
    lens = {len(r) for r in p.reads}
    assert min(lens) == k and max(lens) == k + 40
    assert {(n + 31) // 32 + 1 for n in lens} == {2, 3}
    st = p.o.align(*_pack(p.reads, with_rc=False), m=2, effort=2)[2]
    assert (st == FWD).any() and (st != FWD).any()


@pytest.mark.gpu
@pytest.mark.parametrize("k", sorted(SHORT))
@pytest.mark.parametrize("n", [1, 15, 17, 16 * 14 + 7])
def test_short_reads_small_k(k, n):
    c = _case(("short", k), lambda: _pick_short(k))
    rng = np.random.default_rng(SEED + n)
    lst = [c.p.reads[int(i)] for i in rng.permutation(len(c.p.reads))[:n]]
    c.check("batch%d" % n, *_pack(lst))
    # two words per read: a batch whose longest read has at most 32 bases
    two = [r for r in lst if len(r) <= 32]
    if two:
        c.check("two%d" % n, *_pack(two, with_rc=False), efforts=(0, 2))
