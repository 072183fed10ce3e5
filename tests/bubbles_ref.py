"""Bubbles (`--bubbles`, bgr_bubble, bgr_links_bubbles, bgr_aligner_bubbles, bgr_graph_bubbles, bgr_write_bubbles) in plain Python: the checker of
the product's records and file bytes.  Written from the definition in include/bgreat_gpu.h over links_ref's `counts` dict
({canonical (a, b): traversals}), not from bgreat_amd/.

A bubble is (source, sink, (branch0, branch1), (c0, c1, c2, c3)) with c = the traversals of source -> branch0, branch0 -> sink, source -> branch1,
branch1 -> sink."""
import links_ref


def okey(x):
    """the order of oriented ids: (|x|, x < 0)"""
    return (abs(x), x < 0)


def adjacency(counts, min_link):
    """-> {x: {successor: count}} over the oriented edges of the supported links: (a, b) is a -> b and its strand mate -b -> -a (one edge when b == -a)"""
    assert min_link >= 1
    out = {}
    for (a, b), c in counts.items():
        assert links_ref.canonical(a, b) == (a, b), (a, b)
        if c < min_link:
            continue
        out.setdefault(a, {})[b] = c
        out.setdefault(-b, {})[-a] = c
    return out


def opens(adj, s):
    """-> (s, t, b, c) with b, c in branch order when the oriented s opens a bubble, else None"""
    out = lambda x: adj.get(x, {})
    n_in = lambda x: len(out(-x))
    if len(out(s)) != 2:
        return None
    b, c = sorted(out(s), key=okey)
    if n_in(b) != 1 or n_in(c) != 1 or len(out(b)) != 1 or len(out(c)) != 1:
        return None
    (t,), (t2,) = out(b), out(c)
    if t != t2 or n_in(t) != 2:
        return None
    if len({abs(s), abs(b), abs(c), abs(t)}) != 4:
        return None
    return (s, t, b, c)


def all_oriented(counts, min_link):
    """every (s, t, b, c) that some oriented s opens: both strands of every bubble (the set the canonical filter halves)"""
    adj = adjacency(counts, min_link)
    found = [opens(adj, s) for s in sorted(adj, key=okey)]
    return [f for f in found if f]


def mate(q):
    s, t, b, c = q
    return (-t, -s) + tuple(sorted((-b, -c), key=okey))


def bubbles_of(counts, min_link=1):
    """-> the records, one per bubble: under whichever of (s, t) and (-t, -s) has the smaller key, ordered by (|source|, source < 0)"""
    adj = adjacency(counts, min_link)
    recs = []
    for s, t, b, c in all_oriented(counts, min_link):
        assert links_ref.key(s, t) != links_ref.key(-t, -s)
        if links_ref.key(s, t) > links_ref.key(-t, -s):
            continue
        recs.append((s, t, (b, c), (adj[s][b], adj[b][t], adj[s][c], adj[c][t])))
    return recs


def as_tuples(arr):
    """an array of bgreat_amd.BUBBLE_DTYPE -> the same records"""
    return [(int(r["source"]), int(r["sink"]), (int(r["branch"][0]), int(r["branch"][1])), tuple(int(x) for x in r["count"])) for r in arr]


_COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "a": "t", "c": "g", "g": "c", "t": "a"}


def oriented(unitigs, x):
    """the characters of the oriented id x: unitigs[|x|], reverse-complemented for x < 0"""
    s = unitigs[abs(x)]
    return s if x > 0 else "".join(_COMP.get(ch, ch) for ch in reversed(s))


def compare(x, y):
    """-> (kind, diff) of two oriented branches"""
    if len(x) != len(y):
        return "indel", "."
    d = [i for i in range(len(x)) if x[i] != y[i]]
    if len(d) == 1:
        return "snv", "%d:%s>%s" % (d[0], x[d[0]], y[d[0]])
    return "mnv", "."


def bubbles_text(unitigs, recs):
    """the bytes bgr_write_bubbles writes; `unitigs` is the reference's vector (unitigs[0] == "")"""
    out = ["#source\tsink\tbranch1\tbranch2\tlen1\tlen2\tin1\tout1\tin2\tout2\tkind\tdiff\n"]
    for s, t, (b, c), cnt in recs:
        x, y = oriented(unitigs, b), oriented(unitigs, c)
        kind, diff = compare(x, y)
        out.append("%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%d\t%s\t%s\n" % ((s, t, b, c, len(x), len(y)) + tuple(cnt) + (kind, diff)))
    return "".join(out).encode("latin-1")
