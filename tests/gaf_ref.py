"""The GAF record of a mapped read (`--gaf`, bgr_text_batch.want_output = 3, bgr_aligner_path_stats) in plain Python over str: the checker
of the product's GAF output.  Written from the reference (recoverPath aligner.cpp:270-290, getUnitig :293-301, compactionEnd utils.cpp:171-179,
reverseComplements utils.cpp:52-73, the -c writer alignerGreedy.cpp:394-400) and the GAF column list, not from bgreat_amd/.

A row is (status, path ints) as the batch API returns it: path[0] = offset of the read in its walk, path[1:] = signed 1-based unitig ids.
`unitigs` is the reference's vector: unitigs[0] == "" and unitigs[i] the i-th sequence of the file."""
from wide_greedy_ref import ST_RC, reverse_complements

NO_WALK = None


def load_unitigs(path, k):
    """aligner.cpp:408-420: "" at 0, then the sequence lines of the file (2 lines per record) until the first one shorter than k."""
    out = [""]
    with open(path) as f:
        lines = f.read().split("\n")
    for i in range(1, len(lines), 2):
        if len(lines[i]) < k:
            break
        out.append(lines[i])
    return out


def oriented(unitigs, sid):
    u = unitigs[abs(sid)]
    return u if sid > 0 else reverse_complements(u)


def walk_of(unitigs, k, path):
    """-> (walk, [orientation glued on for path[1:], True = forward]) or NO_WALK ("spells no walk": the -c code's bug-compaction condition)."""
    K1 = k - 1
    n = len(path)
    if n < 2 or any(x == 0 or abs(x) >= len(unitigs) for x in path[1:]):
        return NO_WALK
    walk = oriented(unitigs, path[1])
    orient = [path[1] > 0]
    for x in path[2:]:
        u = oriented(unitigs, x)
        if not walk or not u:
            return NO_WALK
        end = walk[len(walk) - K1:]
        if end == u[:K1]:
            walk += u[K1:]
            orient.append(x > 0)
            continue
        r = reverse_complements(u)
        if end == r[:K1]:
            walk += r[K1:]
            orient.append(not x > 0)
            continue
        return NO_WALK
    if path[0] < 0 or path[0] > len(walk):
        return NO_WALK
    return walk, orient


def spell(unitigs, k, segments):
    """[(forward, id)] in the written order and orientation, glued on k-1 characters: what a reader of the line reconstructs (None: they do not glue)."""
    K1 = k - 1
    out = None
    for fwd, i in segments:
        u = unitigs[i] if fwd else reverse_complements(unitigs[i])
        if out is None:
            out = u
        elif out[len(out) - K1:] == u[:K1]:
            out += u[K1:]
        else:
            return None
    return out


def stats(unitigs, k, read, status, path):
    """-> dict(plen, pstart, pend, qstart, qend, cl, nm, segments, Q) of a mapped read, or NO_WALK."""
    w = walk_of(unitigs, k, path)
    if w is NO_WALK:
        return NO_WALK
    walk, orient = w
    L, plen, off = len(read), len(walk), path[0]
    spelled = walk[off:off + L]
    cl = len(spelled)
    segs = [(o, abs(x)) for o, x in zip(orient, path[1:])]
    if status & ST_RC:  # the path reversed, every orientation flipped: the line describes the read as it stands in the input
        segs = [(not o, i) for o, i in reversed(segs)]
        qs, qe, pstart = L - cl, L, plen - (off + cl)
        Q = reverse_complements(spelled)  # alignerGreedy.cpp:394-400
    else:
        qs, qe, pstart = 0, cl, off
        Q = spelled
    nm = sum(1 for a, b in zip(Q, read[qs:qe]) if a != b)
    return {"plen": plen, "pstart": pstart, "pend": pstart + cl, "qstart": qs, "qend": qe, "cl": cl, "nm": nm, "segments": segs, "Q": Q}


def name_of(header):
    """the header line without its first character ('>' or '@'), up to the first space or tab; '*' if that is empty"""
    n = header[1:]
    for i, c in enumerate(n):
        if c in " \t":
            n = n[:i]
            break
    return n or "*"


def line_of(header, read, s):
    segs = "".join((">" if o else "<") + str(i) for o, i in s["segments"])
    cols = [name_of(header), len(read), s["qstart"], s["qend"], "+", segs, s["plen"], s["pstart"], s["pend"], s["cl"] - s["nm"], s["cl"], 255, "NM:i:%d" % s["nm"]]
    return "\t".join(str(c) for c in cols) + "\n"


def parse_line(line):
    c = line.rstrip("\n").split("\t")
    assert len(c) == 13 and c[4] == "+" and c[11] == "255" and c[12].startswith("NM:i:"), line
    segs, i = [], 0
    s = c[5]
    while i < len(s):
        j = i + 1
        while j < len(s) and s[j].isdigit():
            j += 1
        assert s[i] in "<>" and j > i + 1, line
        segs.append((s[i] == ">", int(s[i + 1:j])))
        i = j
    return {"name": c[0], "qlen": int(c[1]), "qstart": int(c[2]), "qend": int(c[3]), "segments": segs, "plen": int(c[6]), "pstart": int(c[7]),
            "pend": int(c[8]), "matches": int(c[9]), "block": int(c[10]), "nm": int(c[12][5:])}


def gaf_of(unitigs, k, headers, reads, rows):
    """The paths stream of a --gaf run over rows in input order -> (text, index of the first mapped read whose path spells no walk or None);
    like -c, the stream ends in front of such a read."""
    out = []
    for i, (st, path) in enumerate(rows):
        if not path:
            continue
        s = stats(unitigs, k, reads[i], st, path)
        if s is NO_WALK:
            return "".join(out), i
        out.append(line_of(headers[i], reads[i], s))
    return "".join(out), None


def path_stat_row(unitigs, k, read, status, path):
    """bgr_path_stat of one read: (path_len, path_start, aligned, mismatches); zeros for an unmapped read; bit 31 of mismatches = spells no walk."""
    if not path:
        return (0, 0, 0, 0)
    s = stats(unitigs, k, read, status, path)
    if s is NO_WALK:
        return (0, 0, 0, 1 << 31)
    return (s["plen"], s["pstart"], s["cl"], s["nm"])
