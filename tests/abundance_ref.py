"""Per-unitig abundance (`--abundance`, bgr_run_options.abundance, bgr_aligner_abundance) in plain Python: the checker of the product's counts.
Written from the definition in include/bgreat_gpu.h (bgr_run_options.abundance) and from gaf_ref.py's conventions, not from bgreat_amd/.

A row is (status, path ints) as the batch API returns it: path[0] = offset of the read in its walk, path[1:] = signed 1-based unitig ids;
an empty path = not mapped.  `lens[i]` = length of unitig i (lens[0] unused).  A table is a list of [reads, bases, kmers] per unitig id
(entry 0 unused)."""


def unitig_lens(unitigs):
    """the reference's vector (unitigs[0] == "") -> lengths"""
    return [len(u) for u in unitigs]


def valid_id(lens, x):
    """a signed path int names a unitig of the graph (the mapper writes no other; a row somebody else wrote may)"""
    return 0 < abs(x) < len(lens)


def extents(lens, k, path):
    """-> [(s_j, e_j)] of the walk path[1:] spells: s_1 = 0, e_j = s_j + len_j, s_(j+1) = e_j - (k - 1); an id that is 0 or beyond the graph's
    has length 0 in the walk"""
    out, s = [], 0
    for x in path[1:]:
        e = s + (lens[abs(x)] if valid_id(lens, x) else 0)
        out.append((s, e))
        s = e - (k - 1)
    return out


def covered(lens, k, L, path):
    """-> (off, cl): the read covers the walk positions [off, off + cl)"""
    ext = extents(lens, k, path)
    plen = max(e for _, e in ext) if ext else 0   # (e_n -- unless an id outside the graph made the walk step back: then the largest e_j)
    off = path[0]
    return off, max(0, min(L, plen - off))


def occurrences(lens, k, L, path):
    """-> [(unitig id, o_j)] per occurrence of a mapped read's path; an occurrence whose id is 0 or beyond the graph's adds nothing"""
    if len(path) < 2:
        return []
    off, cl = covered(lens, k, L, path)
    return [(abs(x), max(0, min(off + cl, e) - max(off, s))) for x, (s, e) in zip(path[1:], extents(lens, k, path)) if valid_id(lens, x)]


def add_read(table, lens, k, L, path):
    K1 = k - 1
    for i, o in occurrences(lens, k, L, path):
        table[i][0] += 1
        table[i][1] += o
        table[i][2] += max(0, o - K1)


def abundance_of(lens, k, read_lens, rows):
    """-> table over all rows (status is not looked at: neither the strand nor a unitig's orientation enters)"""
    table = [[0, 0, 0] for _ in lens]
    for L, (_, path) in zip(read_lens, rows):
        if path:
            add_read(table, lens, k, L, path)
    return table


def text_of(lens, table):
    """the bytes bgr_write_abundance writes"""
    out = ["#unitig\tlength\treads\tbases\tkmers\n"]
    for i in range(1, len(lens)):
        out.append("%d\t%d\t%d\t%d\t%d\n" % (i, lens[i], table[i][0], table[i][1], table[i][2]))
    return "".join(out).encode()


def parse_text(b):
    """-> (lens, table) with entry 0 unused, from the bytes of an abundance file"""
    lines = b.decode().split("\n")
    assert lines[0] == "#unitig\tlength\treads\tbases\tkmers" and lines[-1] == ""
    lens, table = [0], [[0, 0, 0]]
    for n, ln in enumerate(lines[1:-1], 1):
        c = [int(x) for x in ln.split("\t")]
        assert len(c) == 5 and c[0] == n, ln
        lens.append(c[1])
        table.append(c[2:])
    return lens, table


def ids_in_paths(paths_bytes, n_unitigs):
    """occurrences of every unitig id in the bytes of a paths file (a header line, then "off.id.id." as printPath writes a row):
    the reads column by another road"""
    cnt = [0] * (n_unitigs + 1)
    lines = paths_bytes.decode("latin-1").split("\n")
    for ln in lines[1::2]:
        ints = [int(x) for x in ln.split(".") if x]
        for x in ints[1:]:
            cnt[abs(x)] += 1
    return cnt
