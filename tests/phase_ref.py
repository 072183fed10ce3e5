"""Read-backed phasing of neighbouring bubbles (`--phase`, bgr_phase, bgr_bubbles_phase, bgr_graph_phase, bgr_write_phase) in plain Python: the
checker of the product's records and file bytes.  Written from the definition in include/bgreat_gpu.h over bubbles_ref's records and
triples_ref's `counts` dict, not from bgreat_amd/.

A phase record is (via, source, (in1, in2), (out1, out2), sink, (n11, n12, n21, n22))."""
import bubbles_ref
import links_ref
import triples_ref


def orientations(bubbles):
    """every bubble record read both ways: (s, t, (b, c)) and (-t, -s, (-b, -c)), the branches in (|id|, id < 0) order"""
    out = []
    for s, t, (b, c), _ in bubbles:
        out.append((s, t, tuple(sorted((b, c), key=bubbles_ref.okey))))
        out.append((-t, -s, tuple(sorted((-b, -c), key=bubbles_ref.okey))))
    return out


def phase_of(bubbles, triples):
    """-> the records, one per neighbour pair (X's sink == Y's source == m), in the reading with m > 0, ordered by m"""
    o = orientations(bubbles)
    by_source = {}
    for q in o:
        assert q[0] not in by_source, q   # an oriented id opens at most one bubble
        by_source[q[0]] = q
    recs = []
    for s, m, ins in o:
        if m > 0 and m in by_source:
            _, t, outs = by_source[m]
            n = tuple(triples.get(triples_ref.canonical(i, m, j), 0) for i in ins for j in outs)
            recs.append((m, s, ins, outs, t, n))
    recs.sort(key=lambda r: r[0])
    assert len({r[0] for r in recs}) == len(recs)
    return recs


def call(n):
    cis, trans = n[0] + n[3], n[1] + n[2]
    return "cis" if cis > trans else ("trans" if cis < trans else ".")


def phase_text(recs):
    """the bytes bgr_write_phase writes"""
    out = ["#via\tsource\tin1\tin2\tout1\tout2\tsink\tn11\tn12\tn21\tn22\tphase\n"]
    for m, s, ins, outs, t, n in recs:
        out.append("\t".join(str(x) for x in (m, s) + tuple(ins) + tuple(outs) + (t,) + tuple(n)) + "\t" + call(n) + "\n")
    return "".join(out).encode("latin-1")


def parse_text(b):
    lines = b.decode("latin-1").split("\n")
    assert lines[0] == "#via\tsource\tin1\tin2\tout1\tout2\tsink\tn11\tn12\tn21\tn22\tphase" and lines[-1] == "", lines[:1]
    recs = []
    for ln in lines[1:-1]:
        c = ln.split("\t")
        assert len(c) == 12, ln
        v = [int(x) for x in c[:11]]
        recs.append((v[0], v[1], (v[2], v[3]), (v[4], v[5]), v[6], tuple(v[7:11])))
        assert c[11] == call(recs[-1][5]), ln
    return recs


def bubble_spelling(source, sink, b1, b2):
    """the oriented bubble (source, sink, b1, b2) as the `--bubbles` file spells it: (source, sink, branch1, branch2) under whichever of (s, t) and
    (-t, -s) has the smaller key, the branches in (|id|, id < 0) order"""
    if links_ref.key(source, sink) > links_ref.key(-sink, -source):
        source, sink, b1, b2 = -sink, -source, -b1, -b2
    b1, b2 = sorted((b1, b2), key=bubbles_ref.okey)
    return (source, sink, b1, b2)


def bubbles_of_record(rec):
    """-> the spellings of a phase record's two bubbles (X into via, Y out of it)"""
    m, s, ins, outs, t, _ = rec
    return bubble_spelling(s, m, *ins), bubble_spelling(m, t, *outs)


def as_tuples(arr):
    """an array of bgreat_amd.PHASE_DTYPE -> the same records"""
    return [(int(r["via"]), int(r["source"]), tuple(int(x) for x in r["in"]), tuple(int(x) for x in r["out"]), int(r["sink"]), tuple(int(x) for x in r["count"])) for r in arr]
