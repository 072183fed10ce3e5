"""Links and the GFA file (`--gfa`, bgr_link, bgr_aligner_links, bgr_graph_links, bgr_write_gfa) in plain Python: the checker of the product's
link counts and GFA bytes.  Written from the definitions in include/bgreat_gpu.h and from the conventions of gaf_ref.py and abundance_ref.py,
not from bgreat_amd/.

A row is (status, path ints) as the batch API returns it: path[0] = offset of the read in its walk, path[1:] = signed 1-based unitig ids; an
empty path = not mapped.  A link is a pair (a, b) of signed ids; `counts` is a dict {canonical (a, b): traversals}.  `unitigs` is the
reference's vector (unitigs[0] == ""), `table` abundance_ref's table ([reads, bases, kmers] per unitig id, entry 0 unused)."""


def key(x, y):
    return (abs(x), x < 0, abs(y), y < 0)


def canonical(a, b):
    """(a, b) and (-b, -a) are the same junction read from the two strands: the one with the smaller key stands for both"""
    return (a, b) if key(a, b) <= key(-b, -a) else (-b, -a)


def add_path(counts, path, n_unitigs):
    """every consecutive pair of path[1:] is one traversal; a pair with an id that is 0 or beyond n_unitigs is skipped"""
    for a, b in zip(path[1:], path[2:]):
        if a == 0 or b == 0 or abs(a) > n_unitigs or abs(b) > n_unitigs:
            continue
        c = canonical(a, b)
        counts[c] = counts.get(c, 0) + 1


def links_of(rows, n_unitigs):
    """-> counts over all rows (neither the status nor path[0] is looked at)"""
    counts = {}
    for _, path in rows:
        add_path(counts, path, n_unitigs)
    return counts


def add_counts(a, b):
    out = dict(a)
    for l, c in b.items():
        out[l] = out.get(l, 0) + c
    return out


def sorted_links(counts):
    """-> [(a, b, count)] with count > 0, sorted by key ('+' before '-')"""
    return [(a, b, c) for (a, b), c in sorted(counts.items(), key=lambda kv: key(*kv[0])) if c > 0]


def gfa_text(unitigs, k, table, counts):
    """the bytes bgr_write_gfa writes"""
    out = ["H\tVN:Z:1.0\n"]
    for i in range(1, len(unitigs)):
        out.append("S\t%d\t%s\tLN:i:%d\tRC:i:%d\tKC:i:%d\n" % (i, unitigs[i], len(unitigs[i]), table[i][0], table[i][2]))
    for a, b, c in sorted_links(counts):
        out.append("L\t%d\t%s\t%d\t%s\t%dM\tRC:i:%d\n" % (abs(a), "-" if a < 0 else "+", abs(b), "-" if b < 0 else "+", k - 1, c))
    return "".join(out).encode("latin-1")


def parse_gfa(b):
    """-> (k - 1 or None, [(id, sequence, LN, RC, KC)], {(a, b): count}) from the bytes of a GFA file as bgr_write_gfa writes it"""
    lines = b.decode("latin-1").split("\n")
    assert lines[0] == "H\tVN:Z:1.0" and lines[-1] == ""
    segs, links, k1, seen_l = [], {}, None, False
    for ln in lines[1:-1]:
        c = ln.split("\t")
        if c[0] == "S":
            assert not seen_l and len(c) == 6 and c[3].startswith("LN:i:") and c[4].startswith("RC:i:") and c[5].startswith("KC:i:"), ln
            segs.append((int(c[1]), c[2], int(c[3][5:]), int(c[4][5:]), int(c[5][5:])))
            assert segs[-1][0] == len(segs) and segs[-1][2] == len(c[2]), ln
        else:
            seen_l = True
            assert c[0] == "L" and len(c) == 7 and c[2] in "+-" and c[4] in "+-" and c[5].endswith("M") and c[6].startswith("RC:i:"), ln
            a = int(c[1]) * (-1 if c[2] == "-" else 1)
            d = int(c[3]) * (-1 if c[4] == "-" else 1)
            assert (a, d) not in links and k1 in (None, int(c[5][:-1])), ln
            k1 = int(c[5][:-1])
            links[(a, d)] = int(c[6][5:])
    return k1, segs, links


def gaf_pairs(segments):
    """the consecutive pairs of a GAF line's segments [(forward, id)] as signed ids"""
    ids = [i if fwd else -i for fwd, i in segments]
    return list(zip(ids, ids[1:]))
