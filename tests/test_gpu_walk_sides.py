"""The two-pair walk of the sixteen-reads-per-wave greedy kernel (g2_step, greedy_kernels.hip) against the oracle.

The kernel walks both sides of an anchor at the same time -- lanes 0-1 of a read's quad to the left, lanes 2-3 to the right, each side
cut on its own once its misses pass m -- and settles the read afterwards as the reference's left-then-right walk would end: a left
overflow or failure decides alone, a right overflow goes to the general kernel only when the misses of both sides fit m, and a right
failure or both totals together above m fail the anchor.  The reads here are built to reach each of those rules: substitutions only
left of the first anchor, split between the read's two ends (each side within m, the sum above it), only at the right end; reads that
start at a unitig's first (k-1)-mer (anchor at position 0) or end at a unitig's last one (nothing right of the anchor); long reads on
graphs of short unitigs (more path ints than a side's half of the row), with and without a failing left side; graphs of 2-4 alleles
(halves of 1-4 candidates); k = 8/21/31/32, m = 0..3, and every read with its reverse complement."""
import numpy as np
import pytest

import bgreat_amd as B
import oracle_py
from tools.synth import Synth

COMP = bytes.maketrans(b"ACGTN", b"TGCAN")
SUB = bytes.maketrans(b"ACGT", b"CGTA")
ST_ALIGNED = 2   # status & 3 (oracle and kernel alike): 0 no anchor, 1 anchored but not aligned, 2 aligned; bit 2 = reverse complement tried


def _mutate(r, where):
    r = bytearray(r)
    for p in where:
        r[p] = SUB[r[p]]
    return bytes(r)


def _pack(reads):
    out = []
    for r in reads:
        out.append(r)
        out.append(r.translate(COMP)[::-1])
    roffs = np.zeros(len(out) + 1, dtype=np.uint64)
    roffs[1:] = np.cumsum([len(r) for r in out])
    return np.frombuffer(b"".join(out), dtype=np.uint8), roffs


def _side_reads(s, seqs, offs, k, n, L, m, seed):
    """clean simulated reads of L bases with m + 1 substitutions placed left (first 6 bases), split over both ends, or right (last 6
    bases), or m at the two ends together; plus unitig prefixes and suffixes (anchor at 0, nothing right of the anchor)"""
    rng = np.random.default_rng(seed)
    base, boffs = s.reads(0, n, L, 0, seed + 1)
    out = []
    for i in range(n):
        r = bytes(base[int(boffs[i]):int(boffs[i + 1])])
        kind = i % 5
        lo = [int(x) for x in rng.choice(6, size=min(m + 1, 6), replace=False)]
        hi = [L - 1 - int(x) for x in rng.choice(6, size=min(m + 1, 6), replace=False)]
        nl = (m + 2) // 2
        if kind == 0:
            r = _mutate(r, lo)                           # the left walk fails, the right walk alone would fit
        elif kind == 1:
            r = _mutate(r, lo[:nl] + hi[:m + 1 - nl])    # each side within m, both together above it (m >= 1)
        elif kind == 2:
            r = _mutate(r, hi)                           # the right walk fails
        elif kind == 3:
            r = _mutate(r, lo[:nl] + hi[:max(0, m - nl)])  # both sides together exactly at m
        out.append(r)
    S = bytes(seqs)
    for u in rng.choice(len(offs) - 1, size=n // 4, replace=False):
        a, b = int(offs[u]), int(offs[u + 1])
        if b - a < k + 2:
            continue
        ln = int(rng.integers(k, b - a))
        out.append(S[a:a + ln])        # the read starts at the unitig's first (k-1)-mer: anchor at position 0
        out.append(S[b - ln:b])        # the read ends at the unitig's last (k-1)-mer
    return out


def _check(g, o, reads, roffs, m, e):
    al = B.Aligner(g, 0)
    p1, po1, st1 = al.align(reads, roffs, m=m, effort=e)
    assert al.launch_info()["four_reads_per_wave"]
    p2, po2, st2 = o.align(reads, roffs, m=m, effort=e)
    assert np.array_equal(st1, st2), np.nonzero(st1 != st2)[0][:10]
    assert np.array_equal(po1, po2) and np.array_equal(p1, p2)
    c = al.counters()
    assert c == {**o.counters(), "overlaps": 0}
    return al, c


@pytest.mark.gpu
@pytest.mark.parametrize("seed,k,d,alleles,L,m,e", [
    (1, 31, 140, 2, 150, 2, 2), (2, 31, 60, 3, 150, 0, 1), (3, 32, 40, 4, 250, 3, 2), (4, 21, 30, 4, 200, 1, 2),
    (5, 8, 12, 3, 120, 2, 2), (6, 8, 20, 4, 90, 3, 1), (7, 21, 75, 2, 100, 2, 3), (8, 32, 90, 3, 479, 1, 2)])
def test_walk_sides_match_oracle(seed, k, d, alleles, L, m, e):
    s = Synth(150000, d, alleles, k, 9100 + seed)
    seqs, offs = s.unitigs()
    g = B.Graph.build(k, seqs, offs)
    assert g.info()["has_exceptions"] == 0
    reads, roffs = _pack(_side_reads(s, seqs, offs, k, 4000, L, m, 9200 + seed))
    _, c = _check(g, oracle_py.Oracle(k, seqs, offs), reads, roffs, m, e)
    assert c["aligned"] > c["reads"] // 10


@pytest.mark.gpu
@pytest.mark.parametrize("seed,k,d,m", [(1, 8, 12, 2), (2, 8, 16, 0), (3, 21, 24, 3)])
def test_walk_sides_overflow_match_oracle(seed, k, d, m):
    """long reads on graphs of short unitigs: more right steps than a side's half of the row, with a clean left side (the general
    kernel takes the read) and with a failing left side (the anchor fails: the left side decides)"""
    s = Synth(60000, d, 3, k, 9300 + seed)
    seqs, offs = s.unitigs()
    g = B.Graph.build(k, seqs, offs)
    reads = _side_reads(s, seqs, offs, k, 1500, 479, m, 9400 + seed)
    reads, roffs = _pack(reads)
    al, _ = _check(g, oracle_py.Oracle(k, seqs, offs), reads, roffs, m, 2)
    assert al.pass_counts()[3] > 0   # some reads overflowed their row and went on to the general kernel


@pytest.mark.gpu
def test_walk_sides_overflow_goes_to_general_kernel():
    """clean long reads whose paths do not fit a row (more than 16 ints: their right walks, from anchors near the read's start,
    overflow their half within m): every one of them goes on to the general kernel, as after the sequential walk"""
    k, m = 8, 2
    s = Synth(60000, 12, 2, k, 9501)
    seqs, offs = s.unitigs()
    g = B.Graph.build(k, seqs, offs)
    reads, roffs = s.reads(0, 2000, 479, 0, 9502)
    o = oracle_py.Oracle(k, seqs, offs)
    al, _ = _check(g, o, reads, roffs, m, 1)
    _, po2, st2 = o.align(reads, roffs, m=m, effort=1)
    long_paths = int(np.sum(((st2 & 3) == ST_ALIGNED) & (np.diff(po2.astype(np.int64)) > 16)))
    assert long_paths > 0
    assert al.pass_counts()[3] >= long_paths


def _junction_kmers(seqs, offs, k):
    """the (k-1)-mers the key table holds: the first and last of every unitig, both strands"""
    S, J = bytes(seqs), set()
    for i in range(len(offs) - 1):
        a, b = int(offs[i]), int(offs[i + 1])
        for x in (S[a:a + k - 1], S[b - k + 1:b]):
            J.add(x)
            J.add(x.translate(COMP)[::-1])
    return J


@pytest.mark.gpu
@pytest.mark.parametrize("m", [1, 2, 3])
def test_walk_sides_right_overflow_over_combined_budget_fails_anchor(m):
    """long reads whose left walk and the first right steps each stay within m but together pass it, and whose right walk then
    overflows its half of the row: the sequential walk fails at that right step, before any overflow, so the anchor fails (a follow-up
    item: the reverse complement) and the read does NOT go to the general kernel from its forward item"""
    k = 21
    s = Synth(60000, 24, 2, k, 9600 + m)
    seqs, offs = s.unitigs()
    g = B.Graph.build(k, seqs, offs)
    J = _junction_kmers(seqs, offs, k)
    base, boffs = s.reads(0, 1200, 479, 0, 9700 + m)
    rng = np.random.default_rng(9800 + m)
    out = []
    for i in range(1200):
        r = bytes(base[int(boffs[i]):int(boffs[i + 1])])
        a = next((j for j in range(len(r) - k + 2) if r[j:j + k - 1] in J), None)
        if a is None or a < 2 or a > 60:
            continue
        nl = int(rng.integers(1, min(m, a) + 1))   # left misses, within m
        left = [int(x) for x in rng.choice(a, size=nl, replace=False)]
        right = [a + k - 1 + int(x) for x in rng.choice(24, size=m + 1 - nl, replace=False)]   # early right misses: the sum passes m
        out.append(_mutate(r, left + right))
    assert len(out) > 200
    roffs = np.zeros(len(out) + 1, dtype=np.uint64)
    roffs[1:] = np.cumsum([len(r) for r in out])
    reads = np.frombuffer(b"".join(out), dtype=np.uint8)
    al, _ = _check(g, oracle_py.Oracle(k, seqs, offs), reads, roffs, m, 1)
    # follow-up items of the launch: one per forward item whose anchor failed; were the combined budget not checked on a right overflow,
    # these items would go to the general kernel instead and leave (nearly) none
    assert al.pass_counts()[0] > len(out) // 2, (al.pass_counts(), len(out))
