"""haplotypes_ref.py, the definition of the haplotypes' sequences in plain Python, checked on blocks small enough to spell by hand: a block of one, a
chain, a reversed reading, a ring; the lengths against the formula, the walk strings, and the writer's lines against literal bytes.  CPU only."""
import random

import pytest

import blocks_gen as G
import blocks_ref as BR
import haplotypes_ref as H

ONES = (1, 1, 1, 1)
K = 4


def rc(s):
    return "".join(H.COMPLEMENT[c] for c in reversed(s))


# a genome with two SNV sites, k = 4: flank, two branches of 2k - 1 = 7 that share their first and last k - 1 = 3 with the flanks, flank, ...
F1, F2, F3 = "ACGTTGCA", "GGATCCAT", "TTCAGGCA"
B1 = [F1[-3:] + x + F2[:3] for x in "AC"]
B2 = [F2[-3:] + x + F3[:3] for x in "GT"]
HAP_A = F1 + "A" + F2 + "G" + F3
HAP_B = F1 + "C" + F2 + "T" + F3
UNITIGS = ["", F1, B1[0], B1[1], F2, B2[0], B2[1], F3]   # ids 1 .. 7
BUBBLES = [(1, 4, (2, 3), ONES), (4, 7, (5, 6), ONES)]


def test_a_block_of_one_and_the_formula():
    entries = [(1, 0, 1, 0, 0), (2, 0, 1, 1, 0)]
    recs, data, bad, walks = H.haplotypes_of(UNITIGS, K, BUBBLES, entries)
    assert walks == [[1, 2, 4], [1, 3, 4], [4, 5, 7], [4, 6, 7]] and bad == 0
    assert [data[o:o + n].decode() for _, _, _, _, o, n in recs] == [F1 + "A" + F2, F1 + "C" + F2, F2 + "G" + F3, F2 + "T" + F3]
    assert recs == [(1, 0, 1, 0, 0, 17), (1, 1, 1, 0, 17, 17), (2, 0, 1, 0, 34, 17), (2, 1, 1, 0, 51, 17)]
    assert all(n == 8 + 7 + 8 - 2 * 1 * (K - 1) for *_, n in recs) and len(data) == 68
    assert H.haplotypes_of(UNITIGS, K, BUBBLES, entries, 2) == ([], b"", 0, []) and H.haplotypes_of(UNITIGS, K, [], []) == ([], b"", 0, [])


def test_a_chain_cis_and_trans():
    recs, data, bad, walks = H.haplotypes_of(UNITIGS, K, BUBBLES, [(1, 0, 2, 0, 0), (1, 1, 2, 1, 0)])
    assert walks == [[1, 2, 4, 5, 7], [1, 3, 4, 6, 7]] and bad == 0 and data.decode() == HAP_A + HAP_B
    assert recs == [(1, 0, 2, 0, 0, 26), (1, 1, 2, 0, 26, 26)] and 26 == 3 * 8 + 2 * 7 - 2 * 2 * (K - 1)
    recs, data, bad, walks = H.haplotypes_of(UNITIGS, K, BUBBLES, [(1, 0, 2, 0, 0), (1, 1, 2, 1, BR.HAP)])   # trans: the second bubble's branches swap
    assert walks == [[1, 2, 4, 6, 7], [1, 3, 4, 5, 7]] and data.decode() == F1 + "A" + F2 + "T" + F3 + F1 + "C" + F2 + "G" + F3
    assert H.haplotypes_text(UNITIGS, K, BUBBLES, [(1, 0, 2, 0, 0), (1, 1, 2, 1, 0)]) == (
        b">block1_A bubbles=2 length=26 ring=. walk=>1>2>4>5>7\n" + HAP_A.encode() + b"\n>block1_B bubbles=2 length=26 ring=. walk=>1>3>4>6>7\n" + HAP_B.encode() + b"\n")
    with pytest.raises(AssertionError, match="no decided link"):
        H.haplotypes_of(UNITIGS, K, BUBBLES, [(1, 0, 2, 1, 0), (1, 1, 2, 0, 0)])   # the chain read backwards without its mates


def test_a_reversed_reading_spells_the_other_strand():
    """the block read through the mates, from unitig 7 down to 1: every id negative, the sequences the reverse complements of the haplotypes"""
    entries = [(1, 0, 2, 1, BR.REVERSED), (1, 1, 2, 0, BR.REVERSED)]
    bubbles = BUBBLES
    recs, data, bad, walks = H.haplotypes_of(UNITIGS, K, bubbles, entries)
    assert walks == [[-7, -5, -4, -2, -1], [-7, -6, -4, -3, -1]] and bad == 0
    assert data.decode() == rc(HAP_A) + rc(HAP_B)
    assert H.haplotypes_text(UNITIGS, K, bubbles, entries).startswith(b">block1_A bubbles=2 length=26 ring=. walk=<7<5<4<2<1\n" + rc(HAP_A).encode() + b"\n>block1_B ")
    recs, data, bad, walks = H.haplotypes_of(UNITIGS, K, bubbles, [(1, 0, 2, 1, BR.REVERSED | BR.HAP), (1, 1, 2, 0, BR.REVERSED)])
    assert walks == [[-7, -6, -4, -2, -1], [-7, -5, -4, -3, -1]]


def test_a_ring_is_spelled_as_the_walk_it_was_opened_into():
    """two bubbles 1 -> 4 -> 1: the walk ends in the unitig it began with; the flags travel into the record and the line"""
    ring_f2 = F2[:5] + F1[:3]   # a second flank that leads back into F1
    b1 = [F1[-3:] + x + ring_f2[:3] for x in "AC"]
    b2 = [ring_f2[-3:] + x + F1[:3] for x in "GT"]
    unitigs = ["", F1, b1[0], b1[1], ring_f2, b2[0], b2[1]]
    bubbles = [(1, 4, (2, 3), ONES), (4, 1, (5, 6), ONES)]
    for flags, word in ((BR.CIRCULAR, b"circular"), (BR.CIRCULAR | BR.CONFLICT, b"conflict")):
        entries = [(1, 0, 2, 0, flags), (1, 1, 2, 1, flags)]
        recs, data, bad, walks = H.haplotypes_of(unitigs, K, bubbles, entries)
        assert walks == [[1, 2, 4, 5, 1], [1, 3, 4, 6, 1]] and bad == 0
        want = F1 + "A" + ring_f2 + "G" + F1
        assert data[:recs[0][5]].decode() == want and recs[0] == (1, 0, 2, flags, 0, len(want)) and recs[1][:4] == (1, 1, 2, flags)
        assert H.haplotypes_text(unitigs, K, bubbles, entries).startswith(b">block1_A bubbles=2 length=%d ring=%s walk=>1>2>4>5>1\n" % (len(want), word))


def test_bad_junctions_are_counted_and_the_spelling_stays_defined():
    unitigs = list(UNITIGS)
    unitigs[5] = "AAA" + unitigs[5][3:]   # the second bubble's first branch no longer begins with F2's end
    recs, data, bad, walks = H.haplotypes_of(unitigs, K, BUBBLES, [(1, 0, 2, 0, 0), (1, 1, 2, 1, 0)])
    assert bad == 1 and data.decode() == HAP_A + HAP_B   # (the dropped characters are the ones that differ)
    unitigs[7] = "G" + unitigs[7][1:]   # F3: both walks' last junction
    assert H.haplotypes_of(unitigs, K, BUBBLES, [(1, 0, 2, 0, 0), (1, 1, 2, 1, 0)])[2] == 3


@pytest.mark.parametrize("seed", range(5))
def test_random_crafted_blocks_keep_the_formula(seed):
    rng = random.Random(seed)
    shapes = [("path", 1), ("ring", 3), ("path", 7), ("ring", 2), ("path", 2)]
    bubbles, phase, n_unitigs = G.make(shapes, seed)
    entries = BR.blocks_of(bubbles, phase)
    k = rng.choice((5, 9))
    unitigs = [""] + ["".join(rng.choice("ACGT") for _ in range(rng.choice((k, k + 1, 2 * k - 1, 40)))) for _ in range(n_unitigs)]
    for min_block in (1, 2, 3, 8):
        recs, data, bad, walks = H.haplotypes_of(unitigs, k, bubbles, entries, min_block)
        sizes = sorted(s for kind, s in shapes if s >= min_block)
        assert sorted(r[2] for r in recs if r[1] == 0) == sizes and len(recs) == 2 * len(sizes)
        assert [r[4] for r in recs] == [sum(q[5] for q in recs[:i]) for i in range(len(recs))] and sum(r[5] for r in recs) == len(data)
        for r, w in zip(recs, walks):
            assert len(w) == 2 * r[2] + 1 and r[5] == sum(len(unitigs[abs(x)]) for x in w) - 2 * r[2] * (k - 1)
            assert (w[0] == w[-1]) == bool(r[3] & BR.CIRCULAR)
        text = H.haplotypes_text(unitigs, k, bubbles, entries, min_block)
        assert text.count(b"\n") == 2 * len(recs) and text.count(b">block") == len(recs)
