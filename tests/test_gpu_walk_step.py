"""The walk step of the sixteen-reads-per-wave greedy kernel (g4_step with g4_lean_compare, device_common.h) against the oracle.

The kernel's compare loop has both funnel shift amounts and the addresses worked out once per step, the valid-bases mask as one shift of
the even-bit mask, mismatch bits per 32-bit half, and no exception-plane code: graphs with unitig bases outside ACGT must keep going to
the general kernel (launch_plan.h), which compares through ham_chunk and the exception planes.

The reads here are cut out of longer simulated reads at random starts and lengths, so that the compared windows start and end at every
offset modulo 32 on the read side (and, through the unitigs they cross, on the unitig side); lengths run from k to the 479 bases the
kernel takes, so n covers 1, 31, 32, 33 and the windows of several rounds, in left walks, first right steps and later right steps.
Substitutions go up to m + 1 (mismatch counts at exactly m and m + 1), graphs with 2-4 alleles per site give halves of 1-4 candidates
(the two-lanes-per-candidate form and the one-lane form) and ties between candidates; every read comes with its reverse complement."""
import os

import numpy as np
import pytest

import bgreat_amd as B
import oracle_py
from tools.synth import Synth

GOLD = os.path.join(os.path.dirname(__file__), "golden")
COMP = bytes.maketrans(b"ACGTN", b"TGCAN")
MAX_LEN = 479


def _cut_reads(s, k, n, lmax, max_sub, seed):
    """n reads of random length k .. lmax cut out of simulated reads of lmax bases, each followed by its reverse complement"""
    rng = np.random.default_rng(seed)
    base, boffs = s.reads(0, n, lmax, max_sub, seed + 1)
    out = []
    for i in range(n):
        r = bytes(base[int(boffs[i]):int(boffs[i + 1])])
        ln = int(rng.integers(k, lmax + 1))
        a = int(rng.integers(0, lmax - ln + 1))
        r = r[a:a + ln]
        out.append(r)
        out.append(r.translate(COMP)[::-1])
    roffs = np.zeros(len(out) + 1, dtype=np.uint64)
    roffs[1:] = np.cumsum([len(r) for r in out])
    return np.frombuffer(b"".join(out), dtype=np.uint8), roffs


def _check(g, o, reads, roffs, m, e, multi=True):
    al = B.Aligner(g, 0)
    p1, po1, st1 = al.align(reads, roffs, m=m, effort=e)
    assert al.launch_info()["four_reads_per_wave"] == multi
    p2, po2, st2 = o.align(reads, roffs, m=m, effort=e)
    assert np.array_equal(st1, st2), np.nonzero(st1 != st2)[0][:10]
    assert np.array_equal(po1, po2) and np.array_equal(p1, p2)
    c = al.counters()
    assert c == {**o.counters(), "overlaps": 0}
    return c


@pytest.mark.gpu
@pytest.mark.parametrize("seed,k,lmax,m,e,d,alleles", [
    (1, 31, 150, 2, 2, 60, 2), (2, 31, MAX_LEN, 2, 2, 90, 3), (3, 32, MAX_LEN, 3, 1, 40, 4), (4, 21, 250, 1, 3, 30, 4),
    (5, 8, 90, 2, 2, 12, 3), (6, 31, 100, 0, 1, 50, 2), (7, 21, MAX_LEN, 5, 2, 200, 2), (8, 32, 64, 2, 2, 33, 3)])
def test_walk_step_matches_oracle(seed, k, lmax, m, e, d, alleles):
    s = Synth(120000, d, alleles, k, 8300 + seed)
    seqs, offs = s.unitigs()
    g = B.Graph.build(k, seqs, offs)
    assert g.info()["has_exceptions"] == 0
    reads, roffs = _cut_reads(s, k, 6000, lmax, m + 1, 8400 + seed)
    c = _check(g, oracle_py.Oracle(k, seqs, offs), reads, roffs, m, e)
    assert c["aligned"] > c["reads"] // 10


@pytest.mark.gpu
@pytest.mark.parametrize("seed,k,lmax,m", [(1, 31, 150, 2), (2, 21, MAX_LEN, 4), (3, 8, 80, 1)])
def test_walk_step_exception_bases_match_oracle(seed, k, lmax, m):
    """unitigs with bases outside ACGT (N among them): never the sixteen-reads-per-wave kernel, whose walk step has no exception planes"""
    s = Synth(120000, 3 * k, 3, k, 8500 + seed)
    seqs, offs = s.unitigs()
    seqs = np.array(seqs, dtype=np.uint8, copy=True)
    rng = np.random.default_rng(seed)
    pos = rng.choice(len(seqs), size=len(seqs) // 400, replace=False)
    seqs[pos] = np.frombuffer(b"NRY", dtype=np.uint8)[rng.integers(0, 3, size=len(pos))]
    g = B.Graph.build(k, seqs, offs)
    assert g.info()["has_exceptions"] == 1
    reads, roffs = _cut_reads(s, k, 4000, lmax, m + 1, 8600 + seed)
    _check(g, oracle_py.Oracle(k, seqs, offs), reads, roffs, m, 2, multi=False)


@pytest.mark.gpu
@pytest.mark.parametrize("m,e", [(0, 2), (2, 4)])
def test_walk_step_exception_fixture_matches_oracle(m, e):
    """the degenerate fixture graph with exception bases (k = 5: many short unitigs, long walks): the general kernel, against the oracle"""
    path = os.path.join(GOLD, "deg_unitig_exc.fa")
    g = B.Graph.from_fasta(path, 5)
    assert g.info()["has_exceptions"] == 1
    reads, roffs, _, _ = oracle_py.parse_file(os.path.join(GOLD, "deg_reads.fa"), 5)
    _check(g, oracle_py.Oracle(5, fasta=path), reads, roffs, m, e, multi=False)
