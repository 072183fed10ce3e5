"""A failed first anchor whose next anchor lies in the same scan step, against the oracle, row by row.

The greedy multi kernel's anchor scan reports one hit per item: the first.  When that anchor `a` fails, the item leaves a follow-up item that
resumes at a + 1; the two-scanner scan (key table in LDS) starts it at (a + 1) rounded down to a multiple of 16 with the lanes below a + 1
switched off, the one-item scan (key table in L2) exactly at a + 1.  The next anchor `b` of the strand must then be the follow-up item's
first hit wherever it lies -- also when it lies in the very step [hb, hb + 32) (hb = a rounded down to a multiple of 16) that reported `a`,
which is the shape the reads here have:
  - graphs: a variant site every ~140 bases at k = 31, 21 and 12 (the two anchors of a site lie k apart: at k = 12 a step holds both at
    every residue of a, at k = 21 at residues 0-10, at k = 31 at residue 0 only), and one graph at k = 12 with a site every 13-36 bases
    (anchors of neighbouring sites 1-24 apart);
  - reads picked with the oracle, three kinds: the second anchor maps the read (forward strand not aligned at effort 1, aligned at effort
    2); the second anchor fails too and the read goes on to its reverse complement at effort 2 (which maps there, or fails: both occur);
    the third anchor maps it (not at effort 2, forward at effort 3) -- the first kind where the graph offers it (_buckets);
  - cut in front so that a mod 16 takes every value the graph offers, a + 1 lies below the step's 16-base boundary and on it, and b - a is
    1, 2, 15 and 16 (dense graph), 12 (k = 12), 21 (k = 21) and 31 (k = 31);
  - every set at effort 0-3, m = 2, each read together with its reverse complement, through packed planes (Aligner.align) and ASCII reads
    parked on the device (align_device + fetch), with the key table in LDS (two-scanner scan) and in L2 (one-item scan), and through the
    general kernel (KNOB_GREEDY_FAST), which must give the same rows;
  - batches of 1, 15, 17 and 16 n + 7 reads.
The picker asserts that every listed bucket holds a read; a host-only test runs it without a GPU."""
import numpy as np
import pytest

import bgreat_amd as B
import oracle_py
from tools.synth import Synth
from test_gpu_scan_halves import COMP, _pack

SEED = 1101
EFFORTS = (0, 1, 2, 3)
FWD = B.ST_ALIGNED  # aligned on the forward strand (no ST_RC)
KINDS = ("second", "rc", "third")
#        name: (k, genome, site spacing, reads drawn, the b - a its buckets are about)
GRAPHS = {"k31": (31, 400000, 140, 40000, (31,)),
          "k21": (21, 400000, 140, 30000, (21,)),
          "k12": (12, 400000, 140, 30000, (12,)),
          "dense": (12, 60000, 25, 60000, (1, 2, 15, 16))}
PER_BUCKET = 2


def _same_step(a, b):
    return b - (a & ~15) < 32


def _buckets(name):
    """the buckets the picker must fill: (kind, b - a, a mod 16) -- every residue at which a step holds both anchors for the kind "second",
    and for the other two kinds one residue below the 16-base boundary (a + 1 < hb + 16) and, where the step still holds b, the one on it.
    (The two anchors of ONE site, k apart, offer no read of the kind "second" at k = 31 and 21: none among 200 000 reads drawn -- the walk
    that fails from the anchor in front of a site fails from the one behind it as well.  At k = 12 the first anchor is often a chance
    11-mer, and in the dense graph the two anchors belong to two sites.)"""
    out = []
    for d in GRAPHS[name][4]:
        res = [x for x in range(16) if x + d < 32]
        if name not in ("k31", "k21"):
            out += [("second", d, x) for x in res]
        for kind in ("rc", "third"):
            out.append((kind, d, "below"))
            if 15 in res:
                out.append((kind, d, "on"))
    return out


def _anchors(r, J, k1):
    return [j for j in range(len(r) - k1 + 1) if r[j:j + k1] in J]


def _keys(seqs, offs, k1):
    """every (k-1)-mer that starts or ends a unitig, both orientations: the keys of the table"""
    S = bytes(seqs)
    J = set()
    for i in range(len(offs) - 1):
        lo, hi = int(offs[i]), int(offs[i + 1])
        for x in (S[lo:lo + k1], S[hi - k1:hi]):
            J.add(x)
            J.add(x.translate(COMP)[::-1])
    return J


def _kind(x1, x2, x3):
    if x1 != FWD and x2 == FWD:
        return "second"
    if x2 != FWD and x3 == FWD:
        return "third"
    if x2 & B.ST_RC:
        return "rc"
    return None


class _Picked:
    pass


_PICKED = {}


def _pick(name):
    """the graph `name`, its oracle and {bucket: [reads]} (worked out once per run: the host test and the GPU tests share it)"""
    if name in _PICKED:
        return _PICKED[name]
    k, G, d, n, dists = GRAPHS[name]
    k1 = k - 1
    p = _Picked()
    p.k = k
    s = Synth(G, d, 2, k, SEED + k + d)
    p.seqs, p.offs = s.unitigs()
    p.o = oracle_py.Oracle(k, p.seqs, p.offs)
    p.J = _keys(p.seqs, p.offs, k1)
    base, boffs = s.reads(0, n, 150, 2, SEED + 2)
    st = [p.o.align(base, boffs, m=2, effort=e)[2] for e in (1, 2, 3)]
    cuts = []
    for i in np.nonzero(st[0] != FWD)[0]:
        if _kind(int(st[0][i]), int(st[1][i]), int(st[2][i])) is None:
            continue
        r = bytes(base[int(boffs[i]):int(boffs[i + 1])])
        A = _anchors(r, p.J, k1)
        if len(A) < 2 or A[1] - A[0] not in dists:
            continue
        # every cut that leaves both anchors in one step (checked again by the oracle below: a cut can change what a left walk meets)
        cuts += [r[c:] for c in range(A[0] + 1) if _same_step(A[0] - c, A[1] - c)]
    p.by = {b: [] for b in _buckets(name)}
    if cuts:
        reads, roffs = _pack(cuts, with_rc=False)
        c = [p.o.align(reads, roffs, m=2, effort=e)[2].tolist() for e in (1, 2, 3)]
        for r, x1, x2, x3 in zip(cuts, *c):
            kind = _kind(x1, x2, x3)
            A = _anchors(r, p.J, k1)
            if kind is None or len(A) < 2 or not _same_step(A[0], A[1]):
                continue
            a, dist = A[0], A[1] - A[0]
            where = a % 16 if kind == "second" else ("on" if a % 16 == 15 else "below")
            lst = p.by.get((kind, dist, where))
            if lst is not None and len(lst) < PER_BUCKET:
                lst.append(r)
    empty = [b for b, lst in p.by.items() if not lst]
    assert not empty, (name, empty)  # a condition on the seeds, not a tolerance: the oracle alone fills every bucket
    p.reads = [r for b in sorted(p.by, key=str) for r in p.by[b]]
    _PICKED[name] = p
    return p


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_picked_reads_are_what_they_claim(name):
    """(no GPU) every bucket is filled, and its reads have their first two anchors in one step, at the residue and distance the bucket
    names, with the outcome its kind names; over the graphs, a mod 16 takes every value and b - a every listed one"""
    p = _pick(name)
    k1 = p.k - 1
    for (kind, dist, where), lst in p.by.items():
        assert 1 <= len(lst) <= PER_BUCKET
        reads, roffs = _pack(lst, with_rc=False)
        x = [p.o.align(reads, roffs, m=2, effort=e)[2] for e in (1, 2, 3)]
        for i, r in enumerate(lst):
            A = _anchors(r, p.J, k1)
            a, b = A[0], A[1]
            assert b - a == dist and b - (a & ~15) < 32
            hb2 = (a + 1) & ~15  # where the follow-up item starts: b lies in its first step
            assert b - hb2 < (32 if a % 16 != 15 else 16)
            assert _kind(int(x[0][i]), int(x[1][i]), int(x[2][i])) == kind
            if kind == "second":
                assert a % 16 == where
            else:
                assert (a % 16 == 15) == (where == "on")
                if kind == "third":
                    assert len(A) >= 3
    if name == "k12":
        assert {a for (kind, dist, a) in p.by if kind == "second"} == set(range(16))
    assert len(p.reads) < 400


def test_both_ends_of_the_rc_kind_occur():
    """(no GPU) "the second anchor fails too": over the graphs, the reverse complement then maps some of these reads and fails on others"""
    seen = set()
    for name in sorted(GRAPHS):
        p = _pick(name)
        lst = [r for b, l in p.by.items() if b[0] == "rc" for r in l]
        seen |= set(p.o.align(*_pack(lst, with_rc=False), m=2, effort=2)[2].tolist())
    assert {B.ST_ALIGNED | B.ST_RC, B.ST_FAILED | B.ST_RC} <= seen


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------

class _Case:
    """one graph: three aligners (key table in LDS, key table in L2, general kernel only) and the oracle's rows per read set and effort"""

    def __init__(self, name):
        p = _pick(name)
        self.p = p
        g = B.Graph.build(p.k, p.seqs, p.offs)
        self.lds, self.l2, self.gen = B.Aligner(g, 0), B.Aligner(g, 0), B.Aligner(g, 0)
        self.lds.configure(lds_mphf=2)
        self.l2.configure(lds_mphf=1)
        self.gen.set_knob(B.KNOB_GREEDY_FAST, 1)
        self.want = {}

    def oracle(self, key, reads, roffs, effort):
        if (key, effort) not in self.want:
            self.want[(key, effort)] = self.p.o.align(reads, roffs, m=2, effort=effort)
        return self.want[(key, effort)]

    def check(self, key, reads, roffs, efforts=EFFORTS):
        n = len(roffs) - 1
        for effort in efforts:
            want = self.oracle(key, reads, roffs, effort)
            rows = {}
            for route, al, staged in (("lds", self.lds, True), ("l2", self.l2, False)):
                rows[route, "planes"] = al.align(reads, roffs, m=2, effort=effort)
                info = al.launch_info()
                assert bool(info["mphf_in_lds"]) == staged and info["four_reads_per_wave"], (route, info)
                dr, do = B.DeviceBuffer(0, reads), B.DeviceBuffer(0, roffs)
                try:
                    al.align_device(dr.data_ptr(), do.data_ptr(), n, int(roffs[-1]), int(np.diff(roffs.astype(np.int64)).max()), m=2, effort=effort)
                    rows[route, "ascii"] = al.fetch(n, int(roffs[-1]) + 8 * n + 8)
                    info = al.launch_info()
                finally:
                    dr.free()
                    do.free()
                assert bool(info["mphf_in_lds"]) == staged and info["four_reads_per_wave"], (route, info)
            rows["general", "planes"] = self.gen.align(reads, roffs, m=2, effort=effort)
            assert not self.gen.launch_info()["four_reads_per_wave"]
            for route, (p1, po1, st1) in rows.items():
                assert np.array_equal(st1, want[2]), (route, effort)
                assert np.array_equal(po1, want[1]) and np.array_equal(p1, want[0]), (route, effort)


_CASES = {}


def _case(name):
    if name not in _CASES:
        _CASES[name] = _Case(name)
    return _CASES[name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_second_anchor_in_the_same_step(name):
    c = _case(name)
    reads, roffs = _pack(c.p.reads)
    c.check("all", reads, roffs)
    # what the test is about, said once more on the rows that matter: effort 2 maps the "second" reads on their forward strand, sends the
    # "rc" reads to the other strand, and effort 3 maps the "third" reads forward
    for kind, effort, ok in (("second", 2, lambda st: st == FWD), ("rc", 2, lambda st: (st & B.ST_RC) != 0), ("third", 3, lambda st: st == FWD)):
        lst = [r for b in sorted(c.p.by, key=str) if b[0] == kind for r in c.p.by[b]]
        for al in (c.lds, c.l2):
            _, _, st = al.align(*_pack(lst, with_rc=False), m=2, effort=effort)
            assert ok(st).all(), (kind, effort)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 15, 17, 16 * 2 + 7])
def test_batch_sizes(n):
    c = _case("k12")
    rng = np.random.default_rng(SEED + n)
    order = rng.permutation(len(c.p.reads))
    lst = [c.p.reads[int(i)] for i in order[:n]]
    c.check("batch%d" % n, *_pack(lst, with_rc=False))
    c.check("batch%d rc" % n, *_pack([r.translate(COMP)[::-1] for r in lst], with_rc=False), efforts=(2,))
