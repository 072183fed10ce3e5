"""Crafted inputs of the haplotype-block tests (test_blocks_host.py, test_gpu_blocks.py, tools/blocks_rate.py): chains and rings of bubbles laid out
over fresh unitig ids -- junctions j_0 .. j_L and two branch ids per bubble --, every id given a random sign, the ids permuted so that record order is
unrelated to chain order, the records canonicalised and sorted with bubbles_ref's helpers, the triple counts crafted per neighbour pair and the
phase records made from them with phase_ref.phase_of."""
import random

import bubbles_ref
import links_ref
import phase_ref
import triples_ref

BIG = 2 ** 64 - 1


def layout(shapes, rng, spare=0):
    """shapes: [("path" | "ring", number of bubbles)] -> (bubbles, n_unitigs, groups): the records sorted and canonical; groups[i] = the |via| of
    component i's neighbour pairs in chain order (a ring's last is the pair that closes it)"""
    total = sum((3 * n + 1 if kind == "path" else 3 * n) for kind, n in shapes) + spare
    names = list(range(1, total + 1))
    rng.shuffle(names)
    signed = [x if rng.random() < 0.5 else -x for x in names]
    fresh = iter(signed)
    bubbles, groups = [], []
    for kind, n in shapes:
        assert n >= (2 if kind == "ring" else 1)
        j = [next(fresh) for _ in range(n + 1 if kind == "path" else n)]
        if kind == "ring":
            j.append(j[0])
        for i in range(n):
            q = (j[i], j[i + 1], next(fresh), next(fresh))
            if links_ref.key(q[0], q[1]) > links_ref.key(-q[1], -q[0]):
                q = bubbles_ref.mate(q)
            b, c = sorted(q[2:], key=bubbles_ref.okey)
            bubbles.append((q[0], q[1], (b, c), (1, 1, 1, 1)))
        groups.append([abs(x) for x in (j[1:-1] if kind == "path" else j[1:])])
    bubbles.sort(key=lambda r: bubbles_ref.okey(r[0]))
    return bubbles, total, groups


def counts_for(parity, rng, big=False):
    """four counts of a pair: parity 0 = cis, 1 = trans, None = undecided"""
    x = rng.randrange(0, 4)
    if parity is None:
        return (0, 0, 0, 0) if rng.random() < 0.3 else (x, x + 1, x, x + 1)   # (n11 + n22 == n12 + n21)
    d = rng.randrange(1, 4)
    n = (BIG, BIG, BIG - 1, BIG) if big else (x + d, x, x, x)   # (big: sums beyond 64 bits, cis by one)
    return n if parity == 0 else (n[1], n[0], n[3], n[2])


def phase_with(bubbles, counts_of_via):
    """the phase records of `bubbles` when the pair through m has the counts counts_of_via[m] (n11, n12, n21, n22 in the record's own order)"""
    triples = {}
    for m, s, ins, outs, t, _ in phase_ref.phase_of(bubbles, {}):
        n = counts_of_via[m]
        for i in range(2):
            for k in range(2):
                if n[2 * i + k]:
                    triples[triples_ref.canonical(ins[i], m, outs[k])] = n[2 * i + k]
    recs = phase_ref.phase_of(bubbles, triples)
    assert all(r[5] == tuple(counts_of_via[r[0]]) for r in recs)
    return recs


def make(shapes, seed, undecided=0.0, ring_parity=None, big=0.02, spare=0):
    """-> (bubbles, phase, n_unitigs).  A path's pairs are cis or trans at random, undecided with probability `undecided`; a ring's pairs are all
    decided, with an even (0) or odd (1) number of trans when ring_parity says so."""
    rng = random.Random(seed)
    bubbles, n_unitigs, groups = layout(shapes, rng, spare)
    counts = {}
    for (kind, _), vias in zip(shapes, groups):
        par = [None if kind == "path" and rng.random() < undecided else rng.randrange(2) for _ in vias]
        if kind == "ring" and ring_parity is not None and sum(par) % 2 != ring_parity:
            par[rng.randrange(len(par))] ^= 1
        for m, p in zip(vias, par):
            counts[m] = counts_for(p, rng, big=rng.random() < big)
    return bubbles, phase_with(bubbles, counts), n_unitigs


def bubbles_array(B, bubbles):
    import numpy as np
    a = np.zeros(len(bubbles), dtype=B.BUBBLE_DTYPE)
    for i, (s, t, br, cnt) in enumerate(bubbles):
        a[i] = (s, t, br, cnt)
    return a


def phase_array(B, phase):
    import numpy as np
    a = np.zeros(len(phase), dtype=B.PHASE_DTYPE)
    for i, (m, s, ins, outs, t, n) in enumerate(phase):
        a[i] = (m, s, ins, outs, t, 0, n)
    return a
