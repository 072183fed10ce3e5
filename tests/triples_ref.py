"""Triples and the triples file (`--triples`, bgr_triple, bgr_aligner_triples, bgr_graph_triples, bgr_write_triples) in plain Python: the checker
of the product's triple counts and file bytes.  Written from the definition in include/bgreat_gpu.h and from the conventions of links_ref.py, not
from bgreat_amd/.

A row is (status, path ints) as the batch API returns it: path[0] = offset of the read in its walk, path[1:] = signed 1-based unitig ids; an
empty path = not mapped.  A triple is (a, b, c) of signed ids; `counts` is a dict {canonical (a, b, c): traversals}."""

INT32_MIN = -2 ** 31


def key(a, b, c):
    return (abs(a), a < 0, abs(b), b < 0, abs(c), c < 0)


def canonical(a, b, c):
    """(a, b, c) and (-c, -b, -a) are one triple read from the two strands: the one with the smaller key stands for both (they differ: b != -b)"""
    return (a, b, c) if key(a, b, c) < key(-c, -b, -a) else (-c, -b, -a)


def add_path(counts, path, n_unitigs):
    """every three consecutive ids of path[1:] are one traversal; a triple with an id that is 0 or beyond n_unitigs is skipped"""
    ids = path[1:]
    for a, b, c in zip(ids, ids[1:], ids[2:]):
        a, b, c = int(a), int(b), int(c)
        if any(x == 0 or abs(x) > n_unitigs for x in (a, b, c)):
            continue
        t = canonical(a, b, c)
        counts[t] = counts.get(t, 0) + 1


def triples_of(rows, n_unitigs):
    """-> counts over all rows (neither the status nor path[0] is looked at)"""
    counts = {}
    for _, path in rows:
        add_path(counts, path, n_unitigs)
    return counts


def sorted_triples(counts):
    """-> [(a, b, c, count)] with count > 0, sorted by key"""
    return [t + (n,) for t, n in sorted(counts.items(), key=lambda kv: key(*kv[0])) if n > 0]


def triples_text(counts):
    """the bytes bgr_write_triples writes"""
    return ("#from\tvia\tto\tcount\n" + "".join("%d\t%d\t%d\t%d\n" % t for t in sorted_triples(counts))).encode("latin-1")


def parse_text(b):
    """-> counts from the bytes of a triples file"""
    lines = b.decode("latin-1").split("\n")
    assert lines[0] == "#from\tvia\tto\tcount" and lines[-1] == "", lines[:1]
    counts = {}
    for ln in lines[1:-1]:
        c = ln.split("\t")
        assert len(c) == 4, ln
        t = (int(c[0]), int(c[1]), int(c[2]))
        assert t not in counts and canonical(*t) == t, ln
        counts[t] = int(c[3])
    return counts


def as_tuples(arr):
    """an array of bgreat_amd.TRIPLE_DTYPE -> [(a, b, c, count)]"""
    return [(int(r["from"]), int(r["via"]), int(r["to"]), int(r["count"])) for r in arr]
