"""The fixed-shift window of the two-scanner anchor scan (lds_win32_fixed, key table in LDS) against the oracle, row by row.

A half of the wave starts an item at a multiple of 16 positions, so lane j always holds a position = j mod 16 and reads its (k-1)-mer from
three dwords with shifts that are the lane's constants; a same-strand follow-up item starts at its resume position rounded DOWN to a
multiple of 16, with the lanes below the resume position switched off in its first step.  The reads here are chosen or built so that
  - the first anchor lies at every position 0-64, at each later 16-base boundary and one position either side of it, and at the last
    position of a read (cuts of reads whose first anchor lies further right: the lengths come out mixed, npos <= 16, 17-32, 33-64, > 64);
  - a first anchor that FAILS sits at every position mod 32 and a later anchor of the same strand maps the read (picked with the oracle:
    effort 1 fails the forward strand, effort 2 maps it), so the failed anchor lies in the lanes the follow-up item's first step switches off,
    or just below the block it starts in -- seen again, it would use up the strand's second try (a library built without the lower bound
    in the scan's `valid` fails this test: the forward reads come out FAILED | RC at effort 2; profiles/r10_scan_window_measured.txt);
  - short reads: one position (L = k-1), two, and lengths 1-3 bases either side of the 16- and 32-base boundaries, next to 150-base reads
    in the same wave (the window's third dword then lies in the next read's words or in the zero fill);
  - k = 32 (the widest one-word key: no shift behind the window), 21 and 12 (the longest one);
  - every set through both staging forms: packed planes (Aligner.align) and ASCII reads parked on the device (align_device + fetch);
  - batches of 1, 15, 17 and 16 n + 7 reads.
Effort 0-3 at m = 2, every read together with its reverse complement."""
import numpy as np
import pytest

import bgreat_amd as B
import oracle_py
from tools.synth import Synth
from test_gpu_scan_candidates import K, K1
from test_gpu_scan_halves import COMP, _first_anchor, _junctions, _pack

SEED = 1001
LISTED = tuple(range(65)) + (79, 80, 81, 95, 96, 97, 111, 112, 113)
LAST_AT = (3, 17, 47, 70, 100)  # first anchor = the read's last position, at these positions
EFFORTS = (0, 1, 2, 3)


def _graph(seed=SEED):
    s = Synth(400000, 140, 2, K, seed)
    seqs, offs = s.unitigs()
    return s, seqs, offs


def _boundary_reads(s, seqs, offs, seed=SEED):
    """front cuts of error-free 150-base reads: the first anchor moves to the listed position and stays the first one; three reads per
    position, the third also cut behind (short npos); and reads that end with their first anchor"""
    J = _junctions(seqs, offs)
    base, boffs = s.reads(0, 3000, 150, 0, seed + 1)
    rng = np.random.default_rng(seed)
    src = []
    for i in range(3000):
        r = bytes(base[int(boffs[i]):int(boffs[i + 1])])
        a = _first_anchor(r, J)
        if a is not None:
            src.append((a, r))
    out = []
    for t in LISTED:
        far = [(a, r) for a, r in src if a > t]
        assert len(far) >= 3, t
        pick = rng.choice(len(far), size=3, replace=False)
        for n, j in enumerate(pick):
            a, r = far[int(j)]
            r = r[a - t:]
            if n == 2:
                r = r[:int(rng.integers(t + K1, min(len(r), t + K1 + 40) + 1))]
            out.append(r)
    for t in LAST_AT:
        far = [(a, r) for a, r in src if a > t]
        for j in rng.choice(len(far), size=2, replace=False):
            a, r = far[int(j)]
            out.append(r[a - t:a + K1])
    order = rng.permutation(len(out))
    return [out[i] for i in order]


def _followup_reads(s, seqs, offs, o, seed=SEED):
    """reads whose first forward anchor fails and whose second maps them (the oracle: effort 1 leaves the forward strand, effort 2 aligns on
    it), cut in front so that the failed anchor lies at every position mod 32 -> {position mod 32: [reads]}"""
    if seed in _FOLLOWUPS:  # (worked out once per run: the host test and the GPU test share it)
        return _FOLLOWUPS[seed]
    J = _junctions(seqs, offs)
    base, boffs = s.reads(0, 40000, 150, 2, seed + 2)
    _, _, st1 = o.align(base, boffs, m=2, effort=1)
    _, _, st2 = o.align(base, boffs, m=2, effort=2)
    cand = []
    for i in np.nonzero((st1 != B_ALIGNED) & (st2 == B_ALIGNED))[0]:
        r = bytes(base[int(boffs[i]):int(boffs[i + 1])])
        cand.append((_first_anchor(r, J), r))
    # every cut of every candidate, checked again by the oracle (a cut can change what the left walk of an anchor meets)
    cuts = [r[c:] for a, r in cand for c in range(a + 1)]
    reads, roffs = _pack(cuts, with_rc=False)
    _, _, c1 = o.align(reads, roffs, m=2, effort=1)
    _, _, c2 = o.align(reads, roffs, m=2, effort=2)
    by_res = {}
    for r, x1, x2 in zip(cuts, c1.tolist(), c2.tolist()):
        if x1 != B_ALIGNED and x2 == B_ALIGNED:
            lst = by_res.setdefault(_first_anchor(r, J) % 32, [])
            if len(lst) < 3:
                lst.append(r)
    _FOLLOWUPS[seed] = by_res
    return by_res


_FOLLOWUPS = {}
B_ALIGNED = 2  # BGR_ST_ALIGNED on the forward strand (no BGR_ST_RC)


def _short_reads(s, seqs, offs, seed=SEED):
    """prefixes of reads at the lengths where the window's dwords run out, each next to a 150-base read"""
    J = _junctions(seqs, offs)
    base, boffs = s.reads(0, 1500, 150, 1, seed + 3)
    rng = np.random.default_rng(seed + 3)
    full = [bytes(base[int(boffs[i]):int(boffs[i + 1])]) for i in range(1500)]
    lens = [K1, K1 + 1] + [b + d for b in (32, 48, 64, 80, 96, 112, 128) for d in (-3, -2, -1, 0, 1, 2, 3) if b + d >= K1]
    out = []
    for n, L in enumerate(lens * 3):
        r = full[n]
        a = _first_anchor(r, J)
        if a is not None and n % 3 == 1 and a + K1 >= L:
            r = r[a + K1 - L:]          # the anchor at the read's last position
        elif a is not None and n % 3 == 2 and a < 150 - L:
            r = r[a:]                    # the anchor at its first
        out += [r[:L], full[n + 500]]
    for n in range(40):  # (several short reads side by side: what follows a read's words is the next short read)
        out.append(full[1000 + n][:int(rng.choice(lens))])
    return out


@pytest.fixture(scope="module")
def host_case():
    s, seqs, offs = _graph()
    o = oracle_py.Oracle(K, seqs, offs)
    return s, seqs, offs, o


def test_boundary_reads_are_what_they_claim(host_case):
    """(no GPU) at least two reads with their first anchor at each listed position and at a last position; npos in all four ranges"""
    s, seqs, offs, o = host_case
    reads = _boundary_reads(s, seqs, offs)
    J = _junctions(seqs, offs)
    first = [_first_anchor(r, J) for r in reads]
    for t in LISTED:
        assert sum(1 for a in first if a == t) >= 2, t
    assert sum(1 for a, r in zip(first, reads) if a == len(r) - K1) >= 2
    npos = [len(r) - K1 + 1 for r in reads]
    assert min(npos) >= 1
    assert any(n <= 16 for n in npos) and any(17 <= n <= 32 for n in npos) and any(33 <= n <= 64 for n in npos) and any(n > 64 for n in npos)
    assert len(set(len(r) for r in reads)) > 40 and len(reads) < 4000


def test_followup_reads_are_what_they_claim(host_case):
    """(no GPU) a failed first anchor at every position mod 32 (so every residue mod 16 on both parities), mapped by a later anchor of the
    forward strand: an item that saw the failed anchor twice would spend the second try on it"""
    s, seqs, offs, o = host_case
    by_res = _followup_reads(s, seqs, offs, o)
    assert sorted(by_res) == list(range(32))
    J = _junctions(seqs, offs)
    for res, lst in by_res.items():
        for r in lst:
            anchors = [j for j in range(len(r) - K1 + 1) if r[j:j + K1] in J]
            assert len(anchors) >= 2 and anchors[0] % 32 == res
    reads, roffs = _pack([r for lst in by_res.values() for r in lst], with_rc=False)
    assert (o.align(reads, roffs, m=2, effort=1)[2] != B_ALIGNED).all()
    assert (o.align(reads, roffs, m=2, effort=2)[2] == B_ALIGNED).all()


def test_short_reads_are_what_they_claim(host_case):
    """(no GPU) one and two positions, lengths 1-3 either side of the 16- and 32-base boundaries, each next to a 150-base read"""
    s, seqs, offs, o = host_case
    reads = _short_reads(s, seqs, offs)
    lens = set(len(r) for r in reads)
    assert {K1, K1 + 1} <= lens
    for b in (32, 48, 64, 80, 96, 112, 128):
        assert {b + d for d in (-3, -2, -1, 1, 2, 3) if b + d >= K1} <= lens, b
    assert all(len(reads[i + 1]) == 150 for i in range(0, 2 * 51, 2))


# ---- GPU ---------------------------------------------------------------------------------------------------------------------------------

class _Case:
    """one graph: its aligner (key table staged in LDS) and, per read set and effort, the oracle's rows (worked out once)"""

    def __init__(self, k, seqs, offs):
        self.k = k
        self.al = B.Aligner(B.Graph.build(k, seqs, offs), 0)
        self.al.configure(lds_mphf=2)
        self.o = oracle_py.Oracle(k, seqs, offs)
        self.want = {}

    def oracle(self, name, reads, roffs, effort):
        key = (name, effort)
        if key not in self.want:
            self.want[key] = self.o.align(reads, roffs, m=2, effort=effort)
        return self.want[key]

    def check(self, name, reads, roffs, efforts=EFFORTS, device=True):
        n = len(roffs) - 1
        for effort in efforts:
            p2, po2, st2 = self.oracle(name, reads, roffs, effort)
            # packed planes: <true, 4, false>
            p1, po1, st1 = self.al.align(reads, roffs, m=2, effort=effort)
            info = self.al.launch_info()
            assert info["mphf_in_lds"] and info["four_reads_per_wave"], info
            assert np.array_equal(st1, st2), ("planes", effort)
            assert np.array_equal(po1, po2) and np.array_equal(p1, p2), ("planes", effort)
            if not device:
                continue
            # ASCII reads parked on the device: <true, 4, true>
            dr, do = B.DeviceBuffer(0, reads), B.DeviceBuffer(0, roffs)
            try:
                self.al.align_device(dr.data_ptr(), do.data_ptr(), n, int(roffs[-1]), int(np.diff(roffs.astype(np.int64)).max()), m=2, effort=effort)
                p1, po1, st1 = self.al.fetch(n, int(roffs[-1]) + 8 * n + 8)
                info = self.al.launch_info()
            finally:
                dr.free()
                do.free()
            assert info["mphf_in_lds"] and info["four_reads_per_wave"], info
            assert np.array_equal(st1, st2), ("ascii", effort)
            assert np.array_equal(po1, po2) and np.array_equal(p1, p2), ("ascii", effort)


@pytest.fixture(scope="module")
def case():
    s, seqs, offs = _graph()
    c = _Case(K, seqs, offs)
    c.s, c.seqs, c.offs = s, seqs, offs
    c.boundary = _boundary_reads(s, seqs, offs)
    return c


@pytest.mark.gpu
def test_first_anchor_at_every_boundary(case):
    case.check("boundary", *_pack(case.boundary))


@pytest.mark.gpu
def test_followups_resume_at_every_residue(case):
    by_res = _followup_reads(case.s, case.seqs, case.offs, case.o)
    reads = [r for res in sorted(by_res) for r in by_res[res]]
    reads, roffs = _pack(reads)
    case.check("followup", reads, roffs)
    # what the test is about, said once more on the rows that matter: effort 2 maps every read on its forward strand
    _, _, st = case.al.align(reads, roffs, m=2, effort=2)
    assert (st[0::2] == B_ALIGNED).all()


@pytest.mark.gpu
def test_short_reads_next_to_long_ones(case):
    case.check("short", *_pack(_short_reads(case.s, case.seqs, case.offs)))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 15, 17, 16 * 9 + 7])
def test_batch_sizes_of_the_boundary_set(case, n):
    case.check("batch%d" % n, *_pack(case.boundary[:n], with_rc=False))
    case.check("batch%d rc" % n, *_pack([r.translate(COMP)[::-1] for r in case.boundary[:n]], with_rc=False), efforts=(2,))


def _other_k_case(k):
    G, d = {32: (120000, 90), 21: (120000, 60), 12: (6000, 40)}[k]
    s = Synth(G, d, 2, k, SEED + k)
    seqs, offs = s.unitigs()
    base, boffs = s.reads(0, 600, 150, 2, SEED + k + 1)
    rng = np.random.default_rng(SEED + k)
    reads = []
    for i in range(600):
        r = bytes(base[int(boffs[i]):int(boffs[i + 1])])
        if i % 3 == 1:
            r = r[int(rng.integers(0, 40)):]                       # anchors at other lanes, mixed lengths
        elif i % 3 == 2:
            r = r[:int(rng.integers(k - 1, 151))]                  # down to one position
        reads.append(r)
    return seqs, offs, reads


@pytest.mark.parametrize("k", [32, 21, 12])
def test_other_k_reads_are_what_they_claim(k):
    """(no GPU) the graphs of the other k have keys, and their reads cover one position up to the full length and all three outcomes' worth
    of anchors: most reads map, at effort 2"""
    seqs, offs, reads = _other_k_case(k)
    assert len(offs) - 1 >= 50
    assert min(len(r) for r in reads) == k - 1 or min(len(r) for r in reads) <= k + 2
    o = oracle_py.Oracle(k, seqs, offs)
    _, _, st = o.align(*_pack(reads, with_rc=False), m=2, effort=2)
    assert ((st & 3) == 2).sum() >= len(reads) // 3


@pytest.mark.gpu
@pytest.mark.parametrize("k", [32, 21, 12])
def test_other_k(k):
    seqs, offs, reads = _other_k_case(k)
    c = _Case(k, seqs, offs)
    c.check("k%d" % k, *_pack(reads))
