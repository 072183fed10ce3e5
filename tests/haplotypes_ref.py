"""The haplotypes' sequences (`--haplotypes`, bgr_haplotype, bgr_blocks_haplotypes, bgr_graph_haplotypes, bgr_write_haplotypes) in plain Python: the
checker of the product's records, bytes, bad-junction count and file.  Written from the definition in include/bgreat_gpu.h over bubbles_ref's records
and blocks_ref's entries, not from bgreat_amd/.

unitigs: "" at 0, then the strings (unitig id i is unitigs[i]).  An entry is blocks_ref's (block, index, size, bubble, flags).  Its oriented ids are
(src, snk, a, b) = (source, sink, branch[hap], branch[1 - hap]), with REVERSED (-sink, -source, -branch[hap], -branch[1 - hap]); hap = (flags >> 1) & 1.
A block's walk A is src_0, a_0, snk_0, a_1, snk_1, ..; walk B has b_i for a_i.  The first oriented unitig is spelled whole, every later one without its
first k - 1 characters; a negative id is the reverse complement.  A record is (block, hap, size, ring flags, offset, length)."""
from blocks_ref import CIRCULAR, CONFLICT, REVERSED

COMPLEMENT = {"A": "T", "C": "G", "G": "C", "T": "A"}


def oriented(unitigs, x):
    assert x != 0 and abs(x) < len(unitigs), x
    u = unitigs[abs(x)]
    return u if x > 0 else "".join(COMPLEMENT[c] for c in reversed(u))


def ids_of(entry, bubbles):
    """-> (src, snk, a, b) as the block's reading orients the entry's bubble"""
    s, t, br, _ = bubbles[entry[3]]
    flags = entry[4]
    hap = (flags >> 1) & 1
    return (-t, -s, -br[hap], -br[1 - hap]) if flags & REVERSED else (s, t, br[hap], br[1 - hap])


def blocks_in(entries):
    """the list cut into its blocks, which come one after the other in chain order"""
    out, i = [], 0
    while i < len(entries):
        size = entries[i][2]
        block = entries[i:i + size]
        assert size >= 1 and len(block) == size and [e[1] for e in block] == list(range(size)), entries[i]
        assert len({(e[0], e[2], e[4] & (CIRCULAR | CONFLICT)) for e in block}) == 1, block
        out.append(block)
        i += size
    return out


def walks_of(block, bubbles):
    """-> (walk A, walk B) of one block: 2 n + 1 oriented ids each"""
    ids = [ids_of(e, bubbles) for e in block]
    for p, q in zip(ids, ids[1:]):
        assert p[1] == q[0], "no decided link: an entry's sink is not the next one's source"
    walks = []
    for which in (2, 3):
        w = [ids[0][0]]
        for q in ids:
            w += [q[which], q[1]]
        walks.append(w)
    return tuple(walks)


def spell(unitigs, k, walk):
    """-> (the sequence, its bad junctions)"""
    strings = [oriented(unitigs, x) for x in walk]
    bad = sum(1 for p, c in zip(strings, strings[1:]) if p[len(p) - (k - 1):] != c[:k - 1])
    return strings[0] + "".join(s[k - 1:] for s in strings[1:]), bad


def haplotypes_of(unitigs, k, bubbles, entries, min_block=1):
    """-> (records, bytes, bad junctions, walks): the kept blocks in block order, A before B, the sequences back to back"""
    assert min_block >= 1
    records, parts, walks, bad, offset = [], [], [], 0, 0
    for block in blocks_in(entries):
        number, _, size, _, flags = block[0]
        if size < min_block:
            continue
        for hap, walk in enumerate(walks_of(block, bubbles)):
            s, b = spell(unitigs, k, walk)
            assert len(s) == sum(len(unitigs[abs(x)]) for x in walk) - 2 * size * (k - 1)
            records.append((number, hap, size, flags & (CIRCULAR | CONFLICT), offset, len(s)))
            parts.append(s)
            walks.append(walk)
            bad += b
            offset += len(s)
    return records, "".join(parts).encode("latin-1"), bad, walks


def walk_text(walk):
    return "".join(("<" if x < 0 else ">") + str(abs(x)) for x in walk)


def haplotypes_text(unitigs, k, bubbles, entries, min_block=1):
    """the bytes bgr_write_haplotypes writes"""
    records, data, _, walks = haplotypes_of(unitigs, k, bubbles, entries, min_block)
    out = []
    for (block, hap, size, flags, offset, length), walk in zip(records, walks):
        ring = "conflict" if flags & CONFLICT else ("circular" if flags & CIRCULAR else ".")
        out.append(b">block%d_%s bubbles=%d length=%d ring=%s walk=%s\n" % (block, b"AB"[hap:hap + 1], size, length, ring.encode(), walk_text(walk).encode()))
        out.append(data[offset:offset + length] + b"\n")
    return b"".join(out)


def as_tuples(arr):
    """an array of bgreat_amd.HAPLOTYPE_DTYPE -> the same records"""
    return [(int(r["block"]), int(r["hap"]), int(r["size"]), int(r["flags"]), int(r["offset"]), int(r["length"])) for r in arr]
