"""The two-scanner anchor scan of the sixteen-reads-per-wave greedy kernel (key table in LDS) against the oracle.

With the key table staged in LDS, lanes 0-31 and 32-63 of a wave scan two items at once, 32 positions per step each; a half that has
seen the hits its item needs, or has passed npos, takes the next item of the wave.  The reads here are chosen or built so that:
  - the first anchor lies at positions 30-33 and 62-65 (either side of a half's step boundary), or there is none;
  - read lengths give npos <= 32, 33-64 and > 64, mixed inside one wave, with every read's reverse complement (follow-up items on both
    strands) and substitutions above m (anchors that fail: follow-up items that resume behind them);
  - batches hold 1, 15, 17 and 16 n + 7 reads (a sparse last group of a wave);
  - a read whose only key's first fingerprint candidate fails, with the key behind it (scan_find_key's rare loop), or whose only key
    sits in the fallback list, is scanned by the high half while the low half's read has a hit at its first position in the same step:
    a cut of the candidates by the other half's hit would lose the key, and the read would map as one without an anchor (checked on the
    host with the oracle; the whole-wave cut of the one-read scan fails the GPU test).
Effort 0-3 throughout.  The helpers for the special (k-1)-mers come from tests/test_gpu_scan_candidates.py."""
import numpy as np
import pytest

import bgreat_amd as B
import oracle_py
from tools.synth import Synth
from test_gpu_scan_candidates import K, K1, _case, _dec, _enc, _end_keys, _rc

COMP = bytes.maketrans(b"ACGT", b"TGCA")
SUB = bytes.maketrans(b"ACGT", b"CGTA")
EDGES = (30, 31, 32, 33, 62, 63, 64, 65)


def _pack(reads, with_rc=True):
    out = []
    for r in reads:
        out.append(r)
        if with_rc:
            out.append(r.translate(COMP)[::-1])
    roffs = np.zeros(len(out) + 1, dtype=np.uint64)
    roffs[1:] = np.cumsum([len(r) for r in out])
    return np.frombuffer(b"".join(out), dtype=np.uint8), roffs


def _junctions(seqs, offs):
    """every (k-1)-mer that starts or ends a unitig, both orientations: the keys of the table"""
    S = bytes(seqs)
    J = set()
    for i in range(len(offs) - 1):
        lo, hi = int(offs[i]), int(offs[i + 1])
        for x in (S[lo:lo + K1], S[hi - K1:hi]):
            J.add(x)
            J.add(x.translate(COMP)[::-1])
    return J


def _first_anchor(r, J):
    return next((j for j in range(len(r) - K1 + 1) if r[j:j + K1] in J), None)


def _edge_reads(seed):
    """reads whose first anchor lies at EDGES (several of each), reads without an anchor, and cuts of them to mixed lengths"""
    s = Synth(400000, 140, 2, K, seed)
    seqs, offs = s.unitigs()
    J = _junctions(seqs, offs)
    base, boffs = s.reads(0, 6000, 150, 0, seed + 1)
    rng = np.random.default_rng(seed)
    by_pos = {p: [] for p in EDGES}
    plain = []
    for i in range(6000):
        r = bytes(base[int(boffs[i]):int(boffs[i + 1])])
        a = _first_anchor(r, J)
        if a in by_pos and len(by_pos[a]) < 12:
            by_pos[a].append(r)
        elif len(plain) < 200:
            plain.append(r)
    for p in EDGES:
        assert len(by_pos[p]) >= 4, p
    reads = []
    for p in EDGES:
        for r in by_pos[p]:
            reads.append(r)
            # npos <= 32 / 33-64 / > 64 (the cut keeps the anchor only where it still fits)
            reads.append(r[:int(rng.integers(K1, K1 + 32))])        # npos = L - K1 + 1
            reads.append(r[:int(rng.integers(K1 + 32, K1 + 64))])
            reads.append(r[:int(rng.integers(K1 + 64, 151))])
            # substitutions above m just behind the anchor: the first anchor fails, the next one is tried
            b = bytearray(r)
            for q in range(p + K1, min(p + K1 + 24, 150), 6):
                b[q] = SUB[b[q]]
            reads.append(bytes(b))
    for _ in range(40):  # no anchor at all
        reads.append(bytes(b"ACGT"[c] for c in rng.integers(0, 4, size=int(rng.integers(K1, 151)))))
    reads += plain[:120]
    order = rng.permutation(len(reads))
    return seqs, offs, [reads[i] for i in order]


def _run(al, o, reads, roffs, efforts=(0, 1, 2, 3), m=2):
    for effort in efforts:
        p1, po1, st1 = al.align(reads, roffs, m=m, effort=effort)
        info = al.launch_info()
        assert info["mphf_in_lds"] and info["four_reads_per_wave"], info
        p2, po2, st2 = o.align(reads, roffs, m=m, effort=effort)
        assert np.array_equal(st1, st2), effort
        assert np.array_equal(po1, po2) and np.array_equal(p1, p2), effort


def test_edge_reads_are_what_they_claim():
    """(no GPU) first anchors at each position of EDGES, reads without one, npos in all three ranges"""
    seqs, offs, reads = _edge_reads(901)
    J = _junctions(seqs, offs)
    first = [_first_anchor(r, J) for r in reads]
    for p in EDGES:
        assert sum(1 for a in first if a == p) >= 4, p
    assert sum(1 for a in first if a is None) >= 40
    npos = [len(r) - K1 + 1 for r in reads]
    assert min(npos) >= 1 and any(n <= 32 for n in npos) and any(33 <= n <= 64 for n in npos) and any(n > 64 for n in npos)


@pytest.fixture(scope="module")
def edge_case():
    seqs, offs, reads = _edge_reads(901)
    g = B.Graph.build(K, seqs, offs)
    al = B.Aligner(g, 0)
    al.configure(lds_mphf=2)
    return seqs, offs, reads, al, oracle_py.Oracle(K, seqs, offs)


@pytest.mark.gpu
def test_anchor_at_step_edges_mixed_lengths(edge_case):
    seqs, offs, reads, al, o = edge_case
    _run(al, o, *_pack(reads))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 15, 17, 16 * 37 + 7])
def test_batch_sizes(edge_case, n):
    seqs, offs, reads, al, o = edge_case
    reads = (reads * (n // len(reads) + 1))[:n]
    _run(al, o, *_pack(reads, with_rc=False))
    _run(al, o, *_pack([r.translate(COMP)[::-1] for r in reads], with_rc=False), efforts=(2,))


def _is_key(win, keys):
    return min(_enc(win), _enc(_rc(win))) in keys


def _paired_special_reads(s, seqs, offs, special, cats, seed, scramble=False):
    """pairs of reads, in this order: a unitig start (a hit at position 0: the low half's first step ends at lane 0), then a read made of the
    special (k-1)-mer w at position 1-12 between random bases, w its ONLY key (the high half, whose key must not be cut by lane 0's hit: if it
    were, the read would have no anchor at all).  scramble: w replaced by random bases (what a lost key would map like)."""
    rng = np.random.default_rng(seed)
    keys = _end_keys(seqs, offs)
    n_u = len(offs) - 1
    out = []
    for cat in cats:
        for v in special[cat][:160]:
            w = _dec(v)
            if rng.integers(2):
                w = _rc(w)
            u0 = int(rng.integers(n_u))
            early = bytes(seqs[int(offs[u0]):int(offs[u0 + 1])])[:150]
            while True:
                pre = bytes(b"ACGT"[c] for c in rng.integers(0, 4, size=int(rng.integers(1, 13))))
                tail = bytes(b"ACGT"[c] for c in rng.integers(0, 4, size=150 - K1 - len(pre)))
                late = pre + w + tail
                if not any(_is_key(late[j:j + K1], keys) for j in range(len(late) - K1 + 1) if j != len(pre)):
                    break
            if scramble:
                late = pre + bytes(b"ACGT"[c] for c in rng.integers(0, 4, size=K1)) + tail
            out += [early, late]
    return out


@pytest.mark.parametrize("no_evictions,seed,cats", [
    (False, 31, ("key_behind_false_b1", "key_behind_false_same")),
    (True, 32, ("fallback", "key_behind_false_b1", "key_behind_false_same"))])
def test_high_half_reads_hang_on_their_one_key(no_evictions, seed, cats):
    """(no GPU) each late read's only key is w, and losing w changes what the oracle maps: no anchor instead of a failed one, at every
    effort -- so a cut of the high half's candidates by the low half's hit cannot go unseen"""
    s, seqs, offs, g, special = _case(no_evictions, seed)
    keys = _end_keys(seqs, offs)
    reads = _paired_special_reads(s, seqs, offs, special, cats, seed + 5)
    lost = _paired_special_reads(s, seqs, offs, special, cats, seed + 5, scramble=True)
    late, late_lost = reads[1::2], lost[1::2]
    assert len(late) >= 40
    for r in late:
        assert sum(1 for j in range(len(r) - K1 + 1) if _is_key(r[j:j + K1], keys)) == 1
    o = oracle_py.Oracle(K, seqs, offs)
    for effort in (1, 2, 3):
        _, _, st = o.align(*_pack(late, with_rc=False), m=2, effort=effort)
        _, _, st_lost = o.align(*_pack(late_lost, with_rc=False), m=2, effort=effort)
        assert (st & 3 == 1).all() and (st_lost & 3 == 0).all(), effort  # anchored but not aligned / no anchor at all


@pytest.mark.gpu
@pytest.mark.parametrize("no_evictions,seed,cats", [
    (False, 31, ("key_behind_false_b1", "key_behind_false_same")),
    (True, 32, ("fallback", "key_behind_false_b1", "key_behind_false_same"))])
def test_candidates_of_the_high_half_are_not_cut(no_evictions, seed, cats):
    s, seqs, offs, g, special = _case(no_evictions, seed)
    assert bool(special["fallback"]) == no_evictions
    reads = _paired_special_reads(s, seqs, offs, special, cats, seed + 5)
    al = B.Aligner(g, 0)
    al.configure(lds_mphf=2)
    o = oracle_py.Oracle(K, seqs, offs)
    # in input order (the pairs land in the two halves of a wave's first step) and with each read's reverse complement behind it
    _run(al, o, *_pack(reads, with_rc=False), efforts=(1, 2, 3))
    _run(al, o, *_pack(reads), efforts=(1, 2, 3))
