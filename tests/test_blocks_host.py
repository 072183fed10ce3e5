"""blocks_ref.py, the definition of haplotype blocks in plain Python, checked on cases small enough to chain by hand, and its own assertions (no
component is its own mate, every bubble in exactly one reported block, the mate link keeps the parity) on random crafted inputs.  CPU only."""
import pytest

import blocks_gen as G
import blocks_ref as R
import phase_ref as P

ONES = (1, 1, 1, 1)
CIS, TRANS, NONE = (5, 0, 0, 5), (0, 5, 5, 0), (1, 1, 1, 1)


def rec(via, source, ins, outs, sink, n):
    return (via, source, tuple(ins), tuple(outs), sink, tuple(n))


def test_two_bubbles_cis_and_trans():
    bubbles = [(1, 4, (2, 3), ONES), (4, 7, (5, 6), ONES)]   # nodes 0 = (1, 4), 1 = (-4, -1), 2 = (4, 7), 3 = (-7, -4): 0 -> 2 and 3 -> 1
    assert P.phase_of(bubbles, {}) == [rec(4, 1, (2, 3), (5, 6), 7, (0, 0, 0, 0))]
    assert R.blocks_of(bubbles, [rec(4, 1, (2, 3), (5, 6), 7, CIS)]) == [(1, 0, 2, 0, 0), (1, 1, 2, 1, 0)]
    assert R.blocks_of(bubbles, [rec(4, 1, (2, 3), (5, 6), 7, TRANS)]) == [(1, 0, 2, 0, 0), (1, 1, 2, 1, R.HAP)]
    assert R.blocks_of(bubbles, [rec(4, 1, (2, 3), (5, 6), 7, NONE)]) == [(1, 0, 1, 0, 0), (2, 0, 1, 1, 0)]
    assert R.blocks_of(bubbles, []) == [(1, 0, 1, 0, 0), (2, 0, 1, 1, 0)] and R.blocks_of([], []) == []


def test_three_bubbles_with_an_undecided_pair():
    bubbles = [(1, 4, (2, 3), ONES), (4, 7, (5, 6), ONES), (7, 10, (8, 9), ONES)]
    phase = [rec(4, 1, (2, 3), (5, 6), 7, TRANS), rec(7, 4, (5, 6), (8, 9), 10, NONE)]
    assert R.blocks_of(bubbles, phase) == [(1, 0, 2, 0, 0), (1, 1, 2, 1, R.HAP), (2, 0, 1, 2, 0)]
    phase[1] = rec(7, 4, (5, 6), (8, 9), 10, TRANS)   # trans twice: the third bubble is back on the first one's haplotype
    assert R.blocks_of(bubbles, phase) == [(1, 0, 3, 0, 0), (1, 1, 3, 1, R.HAP), (1, 2, 3, 2, 0)]


def ring_of_three():
    # 1 -> 4 -> 7 -> 1: the third bubble's canonical reading is (-1, -7).  nodes 0 = (1, 4), 1 = (-4, -1), 2 = (-1, -7), 3 = (7, 1), 4 = (4, 7), 5 = (-7, -4);
    # the ring 0 -> 4 -> 3 -> 0 and its mate 1 -> 2 -> 5 -> 1
    bubbles = [(1, 4, (2, 3), ONES), (-1, -7, (-8, -9), ONES), (4, 7, (5, 6), ONES)]
    shape = [rec(1, 7, (8, 9), (2, 3), 4, (0, 0, 0, 0)), rec(4, 1, (2, 3), (5, 6), 7, (0, 0, 0, 0)), rec(7, 4, (5, 6), (8, 9), 1, (0, 0, 0, 0))]
    assert P.phase_of(bubbles, {}) == shape
    return bubbles, shape


def test_rings_of_three():
    bubbles, shape = ring_of_three()
    with_counts = lambda ns: [r[:5] + (n,) for r, n in zip(shape, ns)]
    C = R.CIRCULAR
    assert R.blocks_of(bubbles, with_counts([CIS, CIS, CIS])) == [(1, 0, 3, 0, C), (1, 1, 3, 2, C), (1, 2, 3, 1, C | R.REVERSED)]
    assert R.blocks_of(bubbles, with_counts([TRANS, TRANS, CIS])) == [(1, 0, 3, 0, C), (1, 1, 3, 2, C | R.HAP), (1, 2, 3, 1, C | R.HAP | R.REVERSED)]   # even: the removed link is trans, the last node on B
    X = C | R.CONFLICT
    assert R.blocks_of(bubbles, with_counts([CIS, TRANS, CIS])) == [(1, 0, 3, 0, X), (1, 1, 3, 2, X | R.HAP), (1, 2, 3, 1, X | R.HAP | R.REVERSED)]
    assert R.blocks_of(bubbles, with_counts([TRANS, CIS, CIS])) == [(1, 0, 3, 0, X), (1, 1, 3, 2, X), (1, 2, 3, 1, X | R.REVERSED)]
    # one pair undecided: a path of three, no ring.  Without the pair through 1 it is 0 -> 4 -> 3; without the one through 4 it is 4 -> 3 -> 0, whose
    # mate reading 1 -> 2 -> 5 has the smaller head
    assert R.blocks_of(bubbles, with_counts([NONE, CIS, TRANS])) == [(1, 0, 3, 0, 0), (1, 1, 3, 2, 0), (1, 2, 3, 1, R.HAP | R.REVERSED)]
    assert R.blocks_of(bubbles, with_counts([CIS, NONE, TRANS])) == [(1, 0, 3, 0, R.REVERSED), (1, 1, 3, 1, 0), (1, 2, 3, 2, R.HAP | R.REVERSED)]


def test_a_chain_stored_in_the_mate_reading():
    # (1, -4) and (-7, 4): the shared unitig is walked backwards in both records.  nodes 0 = (1, -4), 1 = (4, -1), 2 = (-7, 4), 3 = (-4, 7): the record
    # is 2 -> 1, its mate link 0 -> 3, and [0, 3] is the reading with the smaller head
    bubbles = [(1, -4, (2, 3), ONES), (-7, 4, (5, 6), ONES)]
    shape = rec(4, -7, (5, 6), (-2, -3), -1, (0, 0, 0, 0))
    assert P.phase_of(bubbles, {}) == [shape]
    assert R.blocks_of(bubbles, [shape[:5] + (CIS,)]) == [(1, 0, 2, 0, 0), (1, 1, 2, 1, R.REVERSED)]
    assert R.blocks_of(bubbles, [shape[:5] + (TRANS,)]) == [(1, 0, 2, 0, 0), (1, 1, 2, 1, R.REVERSED | R.HAP)]


def test_threshold_at_one_below_and_one_above():
    bubbles = [(1, 4, (2, 3), ONES), (4, 7, (5, 6), ONES)]
    phase = [rec(4, 1, (2, 3), (5, 6), 7, (6, 1, 2, 0))]   # cis 6, trans 3
    joined, apart = [(1, 0, 2, 0, 0), (1, 1, 2, 1, 0)], [(1, 0, 1, 0, 0), (2, 0, 1, 1, 0)]
    assert R.blocks_of(bubbles, phase, 2) == joined and R.blocks_of(bubbles, phase, 3) == joined and R.blocks_of(bubbles, phase, 4) == apart
    assert R.decided((G.BIG, G.BIG, G.BIG - 1, G.BIG), 1) == 0 and R.decided((G.BIG, G.BIG, G.BIG - 1, G.BIG), 2) is None and R.decided((0, G.BIG, G.BIG, 0), G.BIG) == 1
    with pytest.raises(AssertionError):
        R.blocks_of(bubbles, phase, 0)


def test_file_bytes():
    bubbles = [(1, -4, (2, 3), ONES), (-7, 4, (5, 6), ONES)]
    entries = R.blocks_of(bubbles, [rec(4, -7, (5, 6), (-2, -3), -1, TRANS)])
    assert R.blocks_text(bubbles, entries) == (b"#block\tindex\tsize\tbubble\tsource\tsink\thapA\thapB\tstrand\tring\n"
                                              b"1\t0\t2\t1\t1\t-4\t2\t3\t+\t.\n"
                                              b"1\t1\t2\t2\t-4\t7\t-6\t-5\t-\t.\n")
    bubbles, shape = ring_of_three()
    entries = R.blocks_of(bubbles, [r[:5] + (n,) for r, n in zip(shape, (CIS, TRANS, CIS))])
    assert R.blocks_text(bubbles, entries) == (b"#block\tindex\tsize\tbubble\tsource\tsink\thapA\thapB\tstrand\tring\n"
                                              b"1\t0\t3\t1\t1\t4\t2\t3\t+\tconflict\n"
                                              b"1\t1\t3\t3\t4\t7\t6\t5\t+\tconflict\n"
                                              b"1\t2\t3\t2\t7\t1\t9\t8\t-\tconflict\n")
    entries = R.blocks_of(bubbles, [r[:5] + (CIS,) for r in shape])
    assert R.blocks_text(bubbles, entries).endswith(b"1\t2\t3\t2\t7\t1\t8\t9\t-\tcircular\n") and R.blocks_text([], []) == R.HEADER.encode()


def test_the_references_own_assertions_on_random_inputs():
    """blocks_of asserts that no component is its own mate, that the mate link keeps the parity and that every bubble lies in exactly one reported
    block; here also: sizes, places and ordinals hang together, and both kinds of ring turn up"""
    import random
    seen = set()
    for seed in range(200):
        rng = random.Random(1000 + seed)
        shapes = [(rng.choice(("path", "path", "ring")), rng.randrange(2, 9)) for _ in range(rng.randrange(1, 7))] + [("path", 1)] * rng.randrange(3)
        bubbles, phase, n_unitigs = G.make(shapes, seed, undecided=0.2)
        for min_phase in (1, 2):
            entries = R.blocks_of(bubbles, phase, min_phase)
            assert len(entries) == len(bubbles)
            at = 0
            for number in range(1, entries[-1][0] + 1):
                size = entries[at][2]
                block = entries[at:at + size]
                assert [e[0] for e in block] == [number] * size and [e[1] for e in block] == list(range(size)) and {e[2] for e in block} == {size}
                assert len({e[4] & (R.CIRCULAR | R.CONFLICT) for e in block}) == 1 and not block[0][4] & R.HAP
                if block[0][4] & R.CIRCULAR:
                    assert not block[0][4] & R.REVERSED   # a ring's first node is its smallest, and of the two readings the even one
                seen.add(block[0][4] & (R.CIRCULAR | R.CONFLICT))
                at += size
            assert at == len(entries)
            firsts = [2 * e[3] + (e[4] & 1) for e in entries if e[1] == 0]
            assert firsts == sorted(firsts)
    assert seen == {0, R.CIRCULAR, R.CIRCULAR | R.CONFLICT}
