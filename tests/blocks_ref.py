"""Haplotype blocks (`--blocks`, bgr_block_entry, bgr_phase_blocks, bgr_graph_blocks, bgr_write_blocks) in plain Python: the checker of the product's
records and file bytes.  Written from the definition in include/bgreat_gpu.h over bubbles_ref's and phase_ref's records, not from bgreat_amd/.

Node 2 i is bubble record i as given, (s, t, b0, b1); node 2 i + 1 its mate (-t, -s, -b0, -b1).  A phase record whose |cis - trans| reaches
min_phase is a decided link X -> Y (X's sink == Y's source == via) with parity 0 (cis) or 1 (trans), and gives the mate link mate(Y) -> mate(X)
with the same parity.  The components are paths and rings; a component and its mate are two readings of one block, reported in the reading whose
first node (a path's head, a ring's smallest node) is smaller.

An entry is (block, index, size, bubble, flags): block 1-based, index and bubble 0-based."""
import bubbles_ref

REVERSED, HAP, CIRCULAR, CONFLICT = 1, 2, 4, 8
HEADER = "#block\tindex\tsize\tbubble\tsource\tsink\thapA\thapB\tstrand\tring\n"


def nodes_of(bubbles):
    out = []
    for s, t, (b0, b1), _ in bubbles:
        assert bubbles_ref.okey(b0) < bubbles_ref.okey(b1) and abs(b0) != abs(b1), (s, t, b0, b1)
        out.append((s, t, b0, b1))
        out.append((-t, -s, -b0, -b1))   # (negating both keeps the (|id|, id < 0) order: |b0| < |b1|)
    return out


def decided(n, min_phase):
    """-> None for an undecided record, else the parity: 0 = cis, 1 = trans (Python's integers: the sums do not wrap)"""
    d = (n[0] + n[3]) - (n[1] + n[2])
    if abs(d) < min_phase:
        return None
    return 0 if d > 0 else 1


def links_of(bubbles, phase, min_phase):
    """-> (nodes, nxt, prv): nxt[x] = (y, parity) or None, prv likewise"""
    assert min_phase >= 1
    nodes = nodes_of(bubbles)
    by_source = {}
    for x, q in enumerate(nodes):
        assert q[0] not in by_source, q
        by_source[q[0]] = x
    nxt, prv = [None] * len(nodes), [None] * len(nodes)
    for m, s, ins, outs, t, n in phase:
        p = decided(n, min_phase)
        assert decided((n[0], n[2], n[1], n[3]), min_phase) == p   # the mate link's counts are the transposed matrix: cis stays cis
        if p is None:
            continue
        x, y = by_source[s], by_source[m]
        assert nodes[x] == (s, m) + tuple(ins) and nodes[y] == (m, t) + tuple(outs), (nodes[x], nodes[y], (m, s, ins, outs, t))
        for a, b in ((x, y), (y ^ 1, x ^ 1)):
            assert nxt[a] is None and prv[b] is None and a != b
            nxt[a], prv[b] = (b, p), (a, p)
    return nodes, nxt, prv


def reading(x, nxt, prv):
    """the component of node x as it is read -> (chain, ring, parity of the link removed from a ring)"""
    seen, h = {x}, x
    while prv[h] is not None and prv[h][0] not in seen:
        h = prv[h][0]
        seen.add(h)
    ring = prv[h] is not None
    if ring:   # (walked all the way round: `seen` is the ring) -- opened at the link that enters its smallest node
        h = min(seen)
    chain = [h]
    while nxt[chain[-1]] is not None and nxt[chain[-1]][0] != h:
        chain.append(nxt[chain[-1]][0])
    return chain, ring, (prv[h][1] if ring else 0)


def blocks_of(bubbles, phase, min_phase=1):
    """-> the entries, block after block, each in chain order"""
    nodes, nxt, prv = links_of(bubbles, phase, min_phase)
    done, found = set(), []
    for x in range(len(nodes)):
        if x in done:
            continue
        a, b = reading(x, nxt, prv), reading(x ^ 1, nxt, prv)
        assert not set(a[0]) & set(b[0]), "a component that is its own mate"
        assert sorted(y ^ 1 for y in a[0]) == sorted(b[0]) and a[1] == b[1]
        if not a[1]:
            assert b[0] == [y ^ 1 for y in reversed(a[0])]
        done |= set(a[0]) | set(b[0])
        found.append(a if a[0][0] < b[0][0] else b)
    found.sort(key=lambda r: r[0][0])
    out = []
    for number, (chain, ring, removed) in enumerate(found, 1):
        hap = 0
        haps = []
        for i, x in enumerate(chain):
            if i:
                hap ^= nxt[chain[i - 1]][1]
            haps.append(hap)
        ringflags = (CIRCULAR | (CONFLICT if removed != haps[-1] else 0)) if ring else 0
        for i, x in enumerate(chain):
            out.append((number, i, len(chain), x >> 1, (x & 1) * REVERSED | haps[i] * HAP | ringflags))
    assert sorted(e[3] for e in out) == list(range(len(bubbles)))   # every bubble record in exactly one reported block, exactly once
    return out


def blocks_text(bubbles, entries):
    """the bytes bgr_write_blocks writes"""
    out = [HEADER]
    for block, index, size, bubble, flags in entries:
        s, t, br, _ = bubbles[bubble]
        hap = (flags >> 1) & 1
        ids = (-t, -s, -br[hap], -br[1 - hap]) if flags & REVERSED else (s, t, br[hap], br[1 - hap])
        ring = "conflict" if flags & CONFLICT else ("circular" if flags & CIRCULAR else ".")
        out.append("%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%s\t%s\n" % ((block, index, size, bubble + 1) + ids + ("-" if flags & REVERSED else "+", ring)))
    return "".join(out).encode("latin-1")


def as_tuples(arr):
    """an array of bgreat_amd.BLOCK_DTYPE -> the same entries"""
    assert not arr["reserved"].any()
    return [(int(r["block"]), int(r["index"]), int(r["size"]), int(r["bubble"]), int(r["flags"])) for r in arr]
