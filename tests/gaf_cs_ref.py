"""The cs:Z: difference string of a GAF line (`--gaf --cs`, bgr_aligner_gaf_cs_enable, bgr_aligner_path_diffs) in plain Python over str, on top
of gaf_ref.py: the checker of the product's field.  minimap2's SHORT cs form, substitutions only (a path and its read have no gaps between them):

    P = gaf_ref.stats(...)["Q"]     the cl characters the path spells under the read, in the read's direction (for a read mapped on its
                                    reverse complement this already is the reversed, complemented spelling)
    R = read[qstart:qend]

walk j = 0 .. cl - 1: equal characters extend a match run; unequal ones first flush a non-empty run as ":<n>" (decimal), then emit
"*" + lower(P[j]) + lower(R[j]); a read character outside ACGT is written "n"; the last run is flushed at the end.  cl == 0 gives the empty value.

The field is "\\tcs:Z:<ops>", the LAST field of the line: behind NM:i: and behind the five haplotag fields where the line carries them.

Invariants (checked by the tests over every row they see):
  * the number of "*" equals NM;
  * the run lengths plus the number of "*" equal column 11 (cl);
  * applying the ops to gaf_ref.spell(segments)[pstart:pend] gives read[qstart:qend], with "n" for every character outside ACGT."""
import gaf_ref as G

ACGT = "ACGT"


def diffs_of(P, R):
    """-> [(j, path base 0..3, read base 0..3 or 4 = outside ACGT)] ascending in j: bgr_path_diff without the read's qstart added"""
    assert len(P) == len(R)
    return [(j, ACGT.index(p), ACGT.index(r) if r in ACGT else 4) for j, (p, r) in enumerate(zip(P, R)) if p != r]


def ops_of(P, R):
    """the value of the field"""
    out, run = [], 0
    for p, r in zip(P, R):
        if p == r:
            run += 1
            continue
        if run:
            out.append(":%d" % run)
            run = 0
        out.append("*" + p.lower() + (r.lower() if r in ACGT else "n"))
    if run:
        out.append(":%d" % run)
    return "".join(out)


def cs_of(read, s):
    """the ops of a mapped read from its gaf_ref.stats"""
    return ops_of(s["Q"], read[s["qstart"]:s["qend"]])


def with_cs(line, ops):
    """a GAF line (plain or tagged) with the field behind everything else"""
    assert line.endswith("\n")
    return line[:-1] + "\tcs:Z:" + ops + "\n"


def parse_ops(ops):
    """-> [("=", n) | ("*", path char, read char)]"""
    out, i = [], 0
    while i < len(ops):
        if ops[i] == ":":
            j = i + 1
            while j < len(ops) and ops[j].isdigit():
                j += 1
            assert j > i + 1 and ops[i + 1] != "0", ops
            out.append(("=", int(ops[i + 1:j])))
            i = j
        else:
            assert ops[i] == "*" and ops[i + 1] in "acgt" and ops[i + 2] in "acgtn" and ops[i + 1] != ops[i + 2], ops
            out.append(("*", ops[i + 1], ops[i + 2]))
            i += 3
    assert all(not (a[0] == "=" and b[0] == "=") for a, b in zip(out, out[1:])), ops   # runs are maximal
    return out


def apply_ops(ops, path_piece):
    """what a reader of the line rebuilds: the read's aligned part from the path's, upper case, 'n' where the read has a character outside ACGT"""
    out, at = [], 0
    for op in parse_ops(ops):
        if op[0] == "=":
            out.append(path_piece[at:at + op[1]])
            at += op[1]
        else:
            assert path_piece[at].lower() == op[1], (ops, at)
            out.append(op[2].upper() if op[2] != "n" else "n")
            at += 1
    assert at == len(path_piece), (ops, at, len(path_piece))
    return "".join(out)


def check_invariants(unitigs, k, read, s, ops):
    """the three invariants of the module's head for one mapped read"""
    p = parse_ops(ops)
    stars = sum(1 for x in p if x[0] == "*")
    assert stars == ops.count("*") == s["nm"]
    assert sum(x[1] for x in p if x[0] == "=") + stars == s["cl"]
    walk = G.spell(unitigs, k, s["segments"])
    piece = read[s["qstart"]:s["qend"]]
    assert apply_ops(ops, walk[s["pstart"]:s["pend"]]) == "".join(c if c in ACGT else "n" for c in piece)


def gaf_cs_of(unitigs, k, headers, reads, rows, tag=None):
    """gaf_ref.gaf_of with the field on every line; tag(line, path) -> line puts the haplotag fields in (or None)"""
    out = []
    for i, (st, path) in enumerate(rows):
        if not path:
            continue
        s = G.stats(unitigs, k, reads[i], st, path)
        if s is G.NO_WALK:
            return "".join(out), i
        line = G.line_of(headers[i], reads[i], s)
        if tag is not None:
            line = tag(line, path)
        out.append(with_cs(line, cs_of(reads[i], s)))
    return "".join(out), None


def path_diff_rows(unitigs, k, read, status, path):
    """bgr_aligner_path_diffs for one read: [(read_pos, path_base, read_base)]; nothing for an unmapped read and for a path that spells no walk"""
    if not path:
        return []
    s = G.stats(unitigs, k, read, status, path)
    if s is G.NO_WALK:
        return []
    return [(s["qstart"] + j, p, r) for j, p, r in diffs_of(s["Q"], read[s["qstart"]:s["qend"]])]
